"""Mirror of coati.generative: embedding, purification, forced decoding (coati_purifications.py) and the embedding-space density fit
(coati_density.py), the nearest-neighbour lookup over an embedding library (coati_search.py; no reference counterpart) and the property-filtered
virtual screen of the reference's generation notebook (coati_screen.py), and guided optimisation of a property in the embedding space
(coati_guide.py; no reference counterpart in the checkout), and diverse picks by clustering the library (coati_cluster.py; no reference
counterpart), and the numeric half of embed_altair.py: a table of embeddings to (X, Y) by exact t-SNE on the GPU (coati_tsne.py), and the library's density as a mixture of diagonal Gaussians that the virtual screen samples from (coati_gmm.py; no reference counterpart).  rdkit is not a dependency: canonicalisation and conformer generation are injected callables."""
from .coati_purifications import decode_most_likely  # noqa: E402,F401
from .coati_search import build_fp4_index, build_index, build_pq_index, drop_near_duplicates, nearest_smiles, smiles_within  # noqa: E402,F401
from .coati_screen import sampled_virtual_screen  # noqa: E402,F401
from .coati_guide import guided_ascent, guided_generation  # noqa: E402,F401
from .coati_cluster import diverse_screen, diverse_subset  # noqa: E402,F401
from .coati_tsne import embed_xy  # noqa: E402,F401
from .coati_gmm import fit_library_density  # noqa: E402,F401
