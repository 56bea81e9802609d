"""The COATI2 TrieTokenizer (simple_coati2/trie_tokenizer.py:11-47): COATI1's tokenizer (the C++ trie of libcoati_hip.so) plus
`n_special` and `mask_token`; a vocabulary without [MASK] is refused with the reference's KeyError."""
from ..encoding.tokenizers.trie_tokenizer import Trie  # noqa: F401
from ..encoding.tokenizers.trie_tokenizer import TrieTokenizer as _TrieTokenizer


class TrieTokenizer(_TrieTokenizer):
    def __init__(self, n_seq=256, smiles_tokens=[], special_tokens=[], side_tasks=True):
        super().__init__(n_seq=n_seq, smiles_tokens=smiles_tokens, special_tokens=special_tokens, side_tasks=side_tasks)
        self.n_special = len(self.special_tokens)
        self.mask_token = self.vocab["[MASK]"]
