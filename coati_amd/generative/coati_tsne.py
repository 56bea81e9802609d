"""The numeric half of the reference's coati.generative.embed_altair: a table of embeddings to one (X, Y) per row by t-SNE, with the
reference's call -- TSNE(n_components=2, learning_rate=100, init="random") -- as the defaults.  The exact method on the GPU
(coati_amd.tsne, EmbeddingIndex.tsne) in place of sklearn's; the chart itself (pandas, altair, the structure tooltips) is not mirrored."""
from typing import Union

import torch

from ..search import EmbeddingIndex


def embed_xy(vectors_or_records: Union[torch.Tensor, list], emb_field: str = "emb", metric: str = "cosine", device="cuda:0",
             **tsne) -> torch.Tensor:
    """[n, 2] f32 (on the CPU): the t-SNE map of vectors [n, dim] -- a tensor or array -- or of the `emb_field` entries of a list of dict
    records, which then also receive "X" and "Y" (floats), as embed_altair's data frame does.  metric: the distance between embeddings,
    "cosine" or "l2" (sklearn's default is euclidean).  **tsne: EmbeddingIndex.tsne's arguments (perplexity, iters, seed, k, ...); lr
    defaults to the reference's 100, init to "random"."""
    records = None
    if isinstance(vectors_or_records, (list, tuple)) and len(vectors_or_records) and isinstance(vectors_or_records[0], dict):
        records = vectors_or_records
        vectors = torch.stack([torch.as_tensor(r[emb_field]).reshape(-1).to(torch.float32) for r in records])
    else:
        vectors = torch.as_tensor(vectors_or_records)
    if vectors.dim() != 2 or vectors.shape[0] < 2:
        raise ValueError(f"embed_xy: embeddings must be [n >= 2, dim], got {tuple(vectors.shape)}")
    tsne.setdefault("lr", 100.0)
    tsne.setdefault("init", "random")
    index = EmbeddingIndex(vectors.shape[1], metric=metric, device=device)
    index.add(vectors)
    xy = index.tsne(**tsne).y.cpu()
    if records is not None:
        for r, (x, y) in zip(records, xy.tolist()):
            r["X"], r["Y"] = x, y
    return xy
