"""Mirror of coati.models.simple_coati2 (COATI2): the SMILES-only inference model COATI_Smiles_Inference with its SwiGLU heads
(transformer_only.py), the checkpoint loader load_coati2 (io.py) and the COATI2 TrieTokenizer (trie_tokenizer.py).  The tensor
maths runs in libcoati_hip.so through coati_amd.engine.Engine (coati_engine_create_coati2)."""
