"""The density of an embedding library as a mixture of diagonal Gaussians (coati_amd.gmm, EmbeddingIndex.gmm): what the virtual screen
samples from when the library, not one Gaussian fitted by estimate_density_batchwise, says where molecules are.  The reference has no
counterpart.

    sampled_virtual_screen(fit_library_density(index, 64), head, model, tokenizer, hit_thresh)"""
import torch

from ..gmm import GaussianMixture
from ..search import EmbeddingIndex


def fit_library_density(index_or_vectors, k: int, **fit) -> GaussianMixture:
    """index.gmm(k, **fit) of an EmbeddingIndex, or of a temporary cosine index over a tensor of vectors [n, dim] (on the GPU the
    vectors are on, else the default one)."""
    if isinstance(index_or_vectors, EmbeddingIndex):
        return index_or_vectors.gmm(k, **fit)
    vectors = torch.as_tensor(index_or_vectors)
    if vectors.dim() != 2:
        raise ValueError(f"fit_library_density: vectors must be [n, dim], got {tuple(vectors.shape)}")
    index = EmbeddingIndex(vectors.shape[1], "cosine", device=vectors.device if vectors.device.type == "cuda" else "cuda:0")
    index.add(vectors)
    return index.gmm(k, **fit)
