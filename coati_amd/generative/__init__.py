"""Mirror of coati.generative: embedding, purification, forced decoding (coati_purifications.py) and the embedding-space density fit
(coati_density.py).  rdkit is not a dependency: canonicalisation and conformer generation are injected callables."""
from .coati_purifications import decode_most_likely  # noqa: E402,F401
