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
                keep_f32: bool = False, nlist: Optional[int] = None, iters: int = 20, seed: int = 0, fp8: bool = False,
                list_dtype: str = "bf16"):
    """An index of the strings' embeddings on the encoder's device and kept, the strings of its rows (kept[i] is row i's, as given).
    Strings that do not canonicalise or tokenize are skipped, as the density fit skips them.  nlist: return a coati_amd.ivf.IVFIndex of
    that many inverted lists over the rows (k-means with `iters`, `seed`) instead of the exact EmbeddingIndex; fp8: return a
    coati_amd.fp8_index.Fp8Index over the rows (e4m3 bytes searched first, the bf16 rows kept for the exact re-ranking); nlist with
    list_dtype="fp8": a coati_amd.ivf8.Ivf8Index, the inverted lists stored as e4m3 bytes and the bf16 rows kept for the re-ranking;
    nlist with list_dtype="pq": a coati_amd.ivfpq.IvfPqIndex, the lists stored as PQ codes of the rows' residuals (code books fitted with
    `seed`, `iters`), the bf16 rows kept likewise; nearest_smiles takes any of them."""
    if list_dtype not in ("bf16", "fp8", "pq"):
        raise ValueError(f'build_index: list_dtype={list_dtype!r} is not "bf16", "fp8" or "pq"')
    if fp8 and nlist is not None:
        raise ValueError('build_index: fp8=True is the exhaustive Fp8Index and nlist= an inverted file; for inverted lists of fp8 rows '
                         'pass nlist= with list_dtype="fp8"')
    if list_dtype != "bf16" and nlist is None:
        raise ValueError(f'build_index: list_dtype="{list_dtype}" needs nlist=')
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
    if nlist is not None and list_dtype == "pq":
        return index.ivfpq(nlist, iters=iters, seed=seed, pq_seed=seed, pq_iters=iters), kept
    if nlist is not None:
        return index.ivf(nlist, iters=iters, seed=seed, fp8=list_dtype == "fp8"), kept
    if fp8:
        return index.fp8(), kept
    return index, kept


def build_pq_index(smiles: Iterable[str], encoder, tokenizer, batch_size: int = 1024, metric: str = "cosine", canon_smiles=None,
                   keep_rows: bool = True, seed: int = 0, iters: int = 20):
    """build_index's rows as a coati_amd.pq.PQIndex and kept, the strings of its rows: one code byte per 8 dimensions under code books
    fitted on the rows (seeded k-means, `iters` rounds); keep_rows=True keeps the bf16 rows for the exact re-ranking, keep_rows=False
    the codes alone.  nearest_smiles takes it."""
    index, kept = build_index(smiles, encoder, tokenizer, batch_size=batch_size, metric=metric, canon_smiles=canon_smiles)
    return index.pq(keep_rows=keep_rows, seed=seed, iters=iters), kept


def build_fp4_index(smiles: Iterable[str], encoder, tokenizer, batch_size: int = 1024, metric: str = "cosine", canon_smiles=None,
                    keep_rows: bool = True):
    """build_index's rows as a coati_amd.fp4_index.Fp4Index and kept, the strings of its rows: e2m1 nibbles with one scale byte per 32
    elements; keep_rows=True keeps the bf16 rows for the exact re-ranking, keep_rows=False the codes and scales alone.  nearest_smiles
    takes it."""
    index, kept = build_index(smiles, encoder, tokenizer, batch_size=batch_size, metric=metric, canon_smiles=canon_smiles)
    return index.fp4(keep_rows=keep_rows), kept


def _query_embeddings(what, queries, index, kept, encoder, tokenizer, canon_smiles):
    """(where, emb): per query its row of emb (None: a string that does not canonicalise or tokenize), emb None when no query is usable"""
    if len(kept) != len(index):
        raise ValueError(f"{what}: {len(kept)} strings for an index of {len(index)} rows")
    if isinstance(queries, torch.Tensor):
        return list(range(queries.shape[0] if queries.dim() == 2 else 1)), queries
    mask = _usable(queries, tokenizer, canon_smiles)
    it = iter(range(sum(mask)))
    where: List[Optional[int]] = [next(it) if ok else None for ok in mask]
    return where, _D._batch_embeds([s for s, ok in zip(queries, mask) if ok], encoder, tokenizer, canon_smiles)


def nearest_smiles(queries: Union[List[str], torch.Tensor], index, kept: List[str], encoder, tokenizer, k: int = 10,
                   canon_smiles=None) -> List[List[Tuple[str, float]]]:
    """Per query its k nearest library strings as (string, score), best first (fewer when the index has fewer rows left).  queries: a
    list of SMILES (one that does not canonicalise or tokenize gets an empty list) or embeddings [Q, E], e.g. encode_points'.  index: an
    EmbeddingIndex, an IVFIndex (then over its default nprobe lists), an Fp8Index, an Fp4Index or a PQIndex (then at its default oversample) or an Ivf8Index or IvfPqIndex (both defaults)."""
    where, emb = _query_embeddings("nearest_smiles", queries, index, kept, encoder, tokenizer, canon_smiles)
    out: List[List[Tuple[str, float]]] = [[] for _ in where]
    if emb is None:
        return out
    scores, rows = index.search(emb, k)
    scores, rows = scores.cpu().tolist(), rows.cpu().tolist()
    for i, w in enumerate(where):
        if w is not None:
            out[i] = [(kept[r], s) for s, r in zip(scores[w], rows[w]) if r >= 0]
    return out


def smiles_within(queries: Union[List[str], torch.Tensor], index, kept: List[str], encoder, tokenizer, threshold: float,
                  canon_smiles=None) -> List[List[Tuple[str, float]]]:
    """Per query ALL library strings whose score reaches `threshold` as (string, score), best first (row ascending among equal scores) --
    nearest_smiles without a k.  threshold is in the units EmbeddingIndex.search returns: cosine or dot score >= threshold; on an "l2"
    index the negated squared distance, so pass -r * r for "within r".  queries: as in nearest_smiles.  index: an EmbeddingIndex, or an
    IVFIndex -- then over the rows of every query's default nprobe nearest lists (IVFIndex.radius_search): a subset of the exact answer
    with the same scores, all of it once nprobe covers the non-empty lists."""
    where, emb = _query_embeddings("smiles_within", queries, index, kept, encoder, tokenizer, canon_smiles)
    out: List[List[Tuple[str, float]]] = [[] for _ in where]
    if emb is None:
        return out
    offsets, scores, rows = index.radius_search(emb, threshold, order="score")
    offsets, scores, rows = offsets.cpu().tolist(), scores.cpu().tolist(), rows.cpu().tolist()
    for i, w in enumerate(where):
        if w is not None:
            out[i] = [(kept[r], s) for s, r in zip(scores[offsets[w]:offsets[w + 1]], rows[offsets[w]:offsets[w + 1]])]
    return out


def drop_near_duplicates(index, kept: List[str], threshold: float, ivf=None, nprobe: int = 8) -> List[int]:
    """Removes from `index` (an EmbeddingIndex) every row that EmbeddingIndex.dedup(threshold) drops -- the later ones of every group of rows
    within the threshold of each other, e.g. one molecule embedded from two spellings -- and returns the row numbers that stay.  Row
    numbers and `kept` do not change (a removed row is only never returned again): kept[i] is still row i's string.
    ivf: an IVFIndex over `index`; the keep mask is then IVFIndex.dedup(threshold, nprobe)'s -- a row looks for earlier neighbours in its
    own and its nprobe - 1 nearest other lists only, so every dropped row is within the threshold of a row that stays, while two rows
    that stay may still be within it if their lists were not probed together -- and the dropped rows are removed from BOTH."""
    if len(kept) != len(index):
        raise ValueError(f"drop_near_duplicates: {len(kept)} strings for an index of {len(index)} rows")
    if ivf is not None and len(ivf) != len(index):
        raise ValueError(f"drop_near_duplicates: an ivf of {len(ivf)} rows for an index of {len(index)} rows")
    live = (index.bias > float("-inf")).cpu()
    if ivf is None:
        keep = index.dedup(threshold).cpu()
    else:
        keep = ivf.dedup(threshold, nprobe=nprobe).cpu()
        stored = torch.zeros(len(ivf), dtype=torch.bool)
        stored[ivf.ids.long().cpu()] = (ivf.bias > float("-inf")).cpu()
        live &= stored                                   # (a row the ivf does not hold is not one it dropped)
    gone = (live & ~keep).nonzero().reshape(-1)
    index.remove(gone)
    if ivf is not None:
        ivf.remove(gone)
    return keep.nonzero().reshape(-1).tolist()
