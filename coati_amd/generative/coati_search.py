"""From SMILES to nearest neighbours: an EmbeddingIndex (coati_amd.search) filled through the packed-row encode, and its lookup by
SMILES or by embedding (a point cloud's, from encode_points: the conformer -> SMILES retrieval the contrastive loss trains for).
Works with a COATI1 model and a COATI_Smiles_Inference alike (the embed helpers tell them apart).  The reference has no counterpart:
its notebooks rank small lists with torch ad hoc."""
from typing import Iterable, List, Optional, Tuple, Union

import torch

from ..common.util import batch_indexable
from ..search import EmbeddingIndex
from . import coati_density as _D
from . import coati_purifications as _P


def _usable(strings, tokenizer, canon_smiles):
    """per string, whether it canonicalises and tokenizes -- whether coati_density._batch_embeds embeds it"""
    canon = _P._canon_fn(canon_smiles)
    mask = []
    for s in strings:
        c = _P._canonical(canon, s)
        mask.append(c is not None and _P._token_row_or_none(tokenizer, c) is not None)
    return mask


def build_index(smiles: Iterable[str], encoder, tokenizer, batch_size: int = 1024, metric: str = "cosine", canon_smiles=None,
                keep_f32: bool = False, nlist: Optional[int] = None, iters: int = 20, seed: int = 0):
    """An index of the strings' embeddings on the encoder's device and kept, the strings of its rows (kept[i] is row i's, as given).
    Strings that do not canonicalise or tokenize are skipped, as the density fit skips them.  nlist: return a coati_amd.ivf.IVFIndex of
    that many inverted lists over the rows (k-means with `iters`, `seed`) instead of the exact EmbeddingIndex; nearest_smiles takes either."""
    index = EmbeddingIndex(encoder.embed_dim, metric=metric, device=encoder.device, keep_f32=keep_f32)
    kept: List[str] = []
    for batch in batch_indexable(smiles, batch_size):
        usable = [s for s, ok in zip(batch, _usable(batch, tokenizer, canon_smiles)) if ok]
        emb = _D._batch_embeds(usable, encoder, tokenizer, canon_smiles)
        if emb is None:
            continue
        if emb.shape[0] != len(usable):
            raise RuntimeError(f"build_index: {len(usable)} usable strings gave {emb.shape[0]} embeddings")
        index.add(emb)
        kept += usable
    if nlist is not None:
        return index.ivf(nlist, iters=iters, seed=seed), kept
    return index, kept


def nearest_smiles(queries: Union[List[str], torch.Tensor], index, kept: List[str], encoder, tokenizer, k: int = 10,
                   canon_smiles=None) -> List[List[Tuple[str, float]]]:
    """Per query its k nearest library strings as (string, score), best first (fewer when the index has fewer rows left).  queries: a
    list of SMILES (one that does not canonicalise or tokenize gets an empty list) or embeddings [Q, E], e.g. encode_points'.  index: an
    EmbeddingIndex or an IVFIndex (then over its default nprobe lists)."""
    if len(kept) != len(index):
        raise ValueError(f"nearest_smiles: {len(kept)} strings for an index of {len(index)} rows")
    if isinstance(queries, torch.Tensor):
        where: List[Optional[int]] = list(range(queries.shape[0] if queries.dim() == 2 else 1))
        emb = queries
    else:
        mask = _usable(queries, tokenizer, canon_smiles)
        it = iter(range(sum(mask)))
        where = [next(it) if ok else None for ok in mask]
        emb = _D._batch_embeds([s for s, ok in zip(queries, mask) if ok], encoder, tokenizer, canon_smiles)
    out: List[List[Tuple[str, float]]] = [[] for _ in where]
    if emb is None:
        return out
    scores, rows = index.search(emb, k)
    scores, rows = scores.cpu().tolist(), rows.cpu().tolist()
    for i, w in enumerate(where):
        if w is not None:
            out[i] = [(kept[r], s) for s, r in zip(scores[w], rows[w]) if r >= 0]
    return out
