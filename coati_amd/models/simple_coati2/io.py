"""COATI2 checkpoint reader with the reference's interface (simple_coati2/io.py:21-91): a pickle document {model_kwargs, model
(state_dict, possibly `module.`-prefixed), train_args["tokenizer_vocab"], ...} -> (COATI_Smiles_Inference, TrieTokenizer).  Local
files only; the model runs on a GPU.  save_coati2 writes such a document (the reference has no writer for COATI2)."""
import pickle

import torch

from ..io.coati import CPU_Unpickler
from .transformer_only import COATI_Smiles_Inference
from .trie_tokenizer import TrieTokenizer


def load_coati2(doc_url: str, device: str = "cuda:0", freeze: bool = True, old_architecture=False, force_cpu=False, vocab=None,
                tokenizer_factory=None, trainable: bool = False):
    """Returns (model, tokenizer).  The tokenizer is TrieTokenizer(n_seq=model_kwargs["n_seq"], **get_vocab(tokenizer_vocab))
    (simple_coati2/io.py:84); `vocab` (a {"special_tokens", "smiles_tokens"} dict or the path of such a JSON file), a directory in
    $COATI_VOCAB_PATH holding <tokenizer_vocab>.json, or `tokenizer_factory(vocab_name, n_seq)` supplies it.  The model gets the
    tokenizer's [PAD] / [STOP] / [UNK] ids.  old_architecture and force_cpu are accepted as in the reference (the first changes
    nothing there either; the document is always read with the CPU unpickler).  trainable is COATI_Smiles_Inference's: True builds
    the engine with gradient and Adam buffers (fine-tuning); it is independent of freeze, which only clears requires_grad."""
    print(f"Loading model from {doc_url}")
    with open(doc_url, "rb") as f_in:
        model_doc = CPU_Unpickler(f_in, encoding="UTF-8").load()
    model_kwargs = model_doc["model_kwargs"]
    state_dict = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in model_doc["model"].items()}
    vocab_name = model_doc["train_args"]["tokenizer_vocab"]
    print(f"Loading tokenizer {vocab_name} from {doc_url}")
    n_seq = model_kwargs["n_seq"]
    if tokenizer_factory is not None:
        tokenizer = tokenizer_factory(vocab_name, n_seq)
    else:
        from ..encoding.tokenizers import get_vocab, load_vocab
        v = load_vocab(vocab) if isinstance(vocab, str) else (vocab if vocab is not None else get_vocab(vocab_name))
        tokenizer = TrieTokenizer(n_seq=n_seq, **v)
    kwargs = {k: model_kwargs[k] for k in ("n_layer_xformer", "n_hidden_xformer", "embed_dim", "n_head", "n_seq", "mlp_dropout",
                                           "enc_to_coati", "n_direct_clr", "n_tok", "biases")}
    model = COATI_Smiles_Inference(**kwargs, device=torch.device(device), dtype=model_kwargs.get("dtype", torch.float),
                                   pad_token=tokenizer.pad_token, stop_token=tokenizer.stop_token, unk_token=tokenizer.unk_token,
                                   trainable=trainable)
    model.load_state_dict(state_dict, strict=False)
    model.device = torch.device(device)
    if freeze:
        n_params = 0
        for param in model.parameters():
            param.requires_grad = False
            n_params += param.numel()
        print(f"{n_params} params frozen!")
    return model, tokenizer


def save_coati2(model, vocab_name: str, path: str, train_args=None):
    """Writes the document load_coati2 reads: {"model_kwargs": model.model_kwargs, "model": the state_dict as CPU tensors (the
    causal-mask buffers included, as torch's state_dict lists them), "train_args": {**train_args, "tokenizer_vocab": vocab_name}}.
    Returns path."""
    doc = {"model_kwargs": dict(model.model_kwargs),
           "model": {k: v.detach().to("cpu").clone() for k, v in model.state_dict().items()},
           "train_args": {**(train_args or {}), "tokenizer_vocab": vocab_name}}
    with open(path, "wb") as f_out:
        pickle.dump(doc, f_out, protocol=pickle.HIGHEST_PROTOCOL)
    return path
