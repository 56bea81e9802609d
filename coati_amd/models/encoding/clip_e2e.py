"""Host-side mirror of the reference's model interface for the hot path (coati/models/encoding/clip_e2e.py):
`e3gnn_smiles_clip_e2e` (same constructor kwargs, attributes, state_dict keys, forward_dist / encode_* signatures),
`clip_loss`, and `clip_ar_xform` (augmentation + tokenisation head over the C++ trie tokenizer, tensorisation tail).  All tensor maths runs in libcoati_hip.so through
coati_amd.engine.Engine; this file only adapts the calling convention."""
import math
from typing import Any, Dict, List

import torch
import torch.nn as nn

from ...engine import Engine, ModelConfig


class _Node(nn.Module):
    """container used to reproduce the reference's dotted state_dict names"""


def _attach(root: nn.Module, dotted: str, tensor: torch.Tensor, grad: torch.Tensor = None, buffer=False):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    if buffer:
        mod.register_buffer(parts[-1], tensor)
    else:
        prm = nn.Parameter(tensor, requires_grad=True)   # shares storage with the flat buffer
        if grad is not None:
            prm.grad = grad
        mod.register_parameter(parts[-1], prm)


def reference_parameter_order(names):
    """The order in which the reference registers its parameters (clip_e2e.py:381-435: point_encoder, xformer, then the
    three heads; inside them e3gnn_clip.py:75-104 and smiles_xformer.py:71-100), i.e. the order of `model.parameters()`
    and therefore of the per-parameter entries of a torch optimizer state_dict written by the reference.  The flat
    device buffers use their own order (transformer first); this is the state_dict / checkpoint contract."""
    def key(n):
        p = n.split(".")
        top = {"point_encoder": 0, "xformer": 1, "point_to_clip": 2, "smiles_to_clip": 3, "point_clip_to_special_tokens": 4}[p[0]]
        wb = {"weight": 0, "bias": 1}[p[-1]]
        if p[0] == "point_encoder":
            if p[1] in ("embedding", "emb"):   # (torch_emb: nn.Embedding `emb` is registered where the Linear `embedding` would be)
                return (top, 0, 0, 0, 0, wb)
            if p[1] == "node_dec":
                return (top, 1, 0, 0, int(p[2]), wb)
            layer = int(p[1].split("_")[1])
            return (top, 2, layer, {"edge_mlp": 0, "node_mlp": 1, "coord_mlp": 2}[p[2]], int(p[3]), wb)
        if p[0] == "xformer":
            if p[1] == "norm_embed":      # norm_embed = True: registered first, never called (smiles_xformer.py:81-84)
                return (top, -1, 0, 0, 0, wb)
            if p[1] == "emb":             # tok_emb.weight, or tok_emb.0.weight / tok_emb.1.{weight, bias} (basic_transformer.py:72-76)
                return (top, 0, 0, 0, int(p[3]) if p[3].isdigit() else 0, wb)
            if p[1] == "lm_head":
                return (top, 3, 0, 0, 0, wb)
            if p[2] == "ln_f":
                return (top, 2, 0, 0, 0, wb)
            layer = int(p[3])
            sub = {"ln_1": (0, 0), "attn": (1, {"c_attn": 0, "c_proj": 1}.get(p[5], 0)), "ln_2": (2, 0),
                   "mlpf": (3, int(p[5]) if p[4] == "mlpf" else 0)}[p[4]]
            return (top, 1, layer, sub[0], sub[1], wb)
        return (top, int(p[1]) if len(p) == 3 else 0, 0, 0, 0, wb)   # (norm_clips=False: a plain Linear, 'point_to_clip.weight')
    return sorted(names, key=key)


class clip_loss(nn.Module):
    """Symmetric InfoNCE with the reference's signature (clip_e2e.py:27-47): returns a [1] tensor.  The value comes
    from the HIP InfoNCE kernels; `backward()` is not wired through autograd -- training uses Engine.train_step."""

    def __init__(self, engine: Engine = None):
        super().__init__()
        object.__setattr__(self, "_engine", engine)

    def forward(self, smiles_features, conformer_features, bad_rows):
        eng = self._engine
        if eng is None:
            raise RuntimeError("clip_loss needs the model's engine: use model.clip_loss")
        s = smiles_features.detach().float().contiguous()
        c = conformer_features.detach().float().contiguous()
        bad = bad_rows.to(torch.uint8).contiguous()
        eng.scal[2:5].zero_()
        eng.infonce(s, c, s, c, bad, row0=0, gscale=1.0)
        sc = eng.scal
        return (0.5 * (sc[2] + sc[3]) / torch.clamp(sc[4], min=1.0)).unsqueeze(0)


def _tokenize_smiles(smi, tokenizer, prefix="[SMILES]", suffix="[STOP]", device="cpu", max_size=None):
    """clip_e2e.py:333-347: the row prefix + smi + suffix zero-padded to max_size (default n_seq), or None when it does not tokenize
    or is longer"""
    if max_size is None:
        max_size = tokenizer.n_seq
    try:
        ttext = tokenizer.tokenize_text(prefix + smi + suffix, pad=False, range_check=False)
        if len(ttext) <= max_size:
            t = torch.zeros(max_size, dtype=torch.long, device=device)
            t[: len(ttext)] = torch.tensor(ttext)
            return t
    except KeyError:
        pass


_LIKELIHOOD_PREFIX = "[CLIP][UNK][SMILES][SUFFIX][MIDDLE]"


def _masked_next_tokens(tokens, tokenizer):
    """the next token of every position ([PAD] behind the last column: the reference's 0 is its [PAD] id, a COATI2 vocabulary has
    another token there); [CLIP] / [PAD] / [SMILES] / [UNK] / [SUFFIX] / [MIDDLE] targets are -1 (clip_e2e.py:647-654)"""
    y_next = torch.full_like(tokens, tokenizer.pad_token)
    y_next[:, : (tokens.shape[1] - 1)] = tokens[:, 1:].clone()
    for t in (tokenizer.clip_token, tokenizer.pad_token, tokenizer.smiles_token, tokenizer.unk_token, tokenizer.suffix_token,
              tokenizer.middle_token):
        y_next[y_next == t] = -1
    return y_next


def _rows_to_tokens(rows, pad_token):
    tokens = torch.full((len(rows), max(len(r) for r in rows)), pad_token, dtype=torch.long)
    for i, r in enumerate(rows):
        tokens[i, : len(r)] = torch.tensor(r, dtype=torch.long)
    return tokens


def hclip_likelihood_tokens(smiles: List[str], tokenizer):
    """Host-side rows of hclip_and_tokens_to_likelihood (clip_e2e.py:638-655) for a list of SMILES: tokens
    [CLIP][UNK][SMILES][SUFFIX][MIDDLE]<smi>[STOP] [B, T] (rows of different length end in [PAD]) and their targets (the next token;
    [CLIP] / [PAD] / [SMILES] / [UNK] / [SUFFIX] / [MIDDLE] targets are -1).  Tokenizer errors propagate as in the reference."""
    tokens = _rows_to_tokens([tokenizer.tokenize_text(_LIKELIHOOD_PREFIX + smi + "[STOP]", pad=False) for smi in smiles], tokenizer.pad_token)
    return tokens, _masked_next_tokens(tokens, tokenizer)


def hcoati_likelihood_tokens(smiles: List[str], tokenizer, do_suffix: bool = False):
    """The COATI2 twin of hclip_likelihood_tokens: rows [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smi>[STOP] -- the prompt hcoati_to_2d
    decodes from (injection_prefix) and the string behind it -- padded with the tokenizer's [PAD], and their targets, masked alike."""
    prefix = injection_prefix(tokenizer, "[SMILES]", do_suffix)
    tokens = _rows_to_tokens([prefix + tokenizer.tokenize_text(smi + "[STOP]", pad=False) for smi in smiles], tokenizer.pad_token)
    return tokens, _masked_next_tokens(tokens, tokenizer)


def s2s_hcoati_likelihood_tokens(smiles: List[str], tokenizer, do_suffix: bool = False):
    """The COATI2 twin of s2s_likelihood_tokens: the mask of the SMILES whose <smi>[STOP] tokenizes and fits n_seq minus the prompt, and for
    those rows the encoder's [SMILES]<smi>[STOP] [n_ok, T1] and the decoder's rows and targets of hcoati_likelihood_tokens, all padded with
    the tokenizer's [PAD].  No row fits: empty tensors and an all-False mask."""
    prefix = injection_prefix(tokenizer, "[SMILES]", do_suffix)
    room = tokenizer.n_seq - len(prefix)
    bodies = []
    for smi in smiles:
        try:
            ids = tokenizer.tokenize_text(smi + "[STOP]", pad=False, range_check=False)
        except KeyError:
            ids = None
        bodies.append(ids if ids is not None and len(ids) <= room else None)
    mask = torch.tensor([b is not None for b in bodies], dtype=torch.bool)
    ok = [b for b in bodies if b is not None]
    if not ok:
        empty = torch.zeros(0, 1, dtype=torch.long)
        return empty, empty, empty, mask
    raw_tokens = _rows_to_tokens([[int(tokenizer.smiles_token)] + b for b in ok], tokenizer.pad_token)
    tokens = _rows_to_tokens([prefix + b for b in ok], tokenizer.pad_token)
    return raw_tokens, tokens, _masked_next_tokens(tokens, tokenizer), mask


def s2s_likelihood_tokens(smiles: List[str], tokenizer):
    """Host-side tensors of batch_smiles_to_s2s_likelihood (clip_e2e.py:670-735): the mask of the SMILES that tokenize into n_seq - 5
    positions, and for those rows the encoder's [SMILES]<smi>[STOP] [n_ok, n_seq - 4], the decoder's
    [CLIP][UNK][SMILES][SUFFIX][MIDDLE]<smi>[STOP] [n_ok, n_seq] and its targets (positions :4, the last column and [PAD] are -1)."""
    _tokens = [_tokenize_smiles(smi, tokenizer, prefix="", suffix="[STOP]", max_size=(tokenizer.n_seq - 5)) for smi in smiles]
    mask = torch.tensor([t is not None for t in _tokens], dtype=torch.bool)
    _tokens = torch.stack([t for t in _tokens if t is not None])
    n = _tokens.shape[0]
    raw_tokens = torch.zeros(n, _tokens.shape[1] + 1, dtype=torch.long)
    raw_tokens[:, 0] = tokenizer.smiles_token
    raw_tokens[:, 1:] = _tokens
    tokens = torch.zeros(n, _tokens.shape[1] + 5, dtype=torch.long)
    for i, t in enumerate((tokenizer.clip_token, tokenizer.unk_token, tokenizer.smiles_token, tokenizer.suffix_token,
                           tokenizer.middle_token)):
        tokens[:, i] = t
    tokens[:, 5:] = _tokens
    y_next = torch.zeros_like(tokens)
    y_next[:, : (tokens.shape[1] - 1)] = tokens[:, 1:].clone()
    y_next[:, :4] = -1
    y_next[:, -1] = -1
    y_next[y_next == tokenizer.pad_token] = -1
    return raw_tokens, tokens, y_next, mask


@torch.no_grad()
def torch_default_init(model: nn.Module, seed, is_layernorm):
    """torch.nn default initialisers over model.named_parameters() in order, drawn from one CPU generator seeded with `seed`
    (default torch.initial_seed()): Linear: kaiming-uniform(a=sqrt 5) weight and U(+-1/sqrt(fan_in)) bias; Embedding: N(0,1);
    LayerNorm (the 1-D parameters `is_layernorm(name)` names): 1/0; coord_mlp.2: xavier-uniform gain 1e-3.  Then the engine's
    shadows are refreshed."""
    g = torch.Generator(device="cpu")
    g.manual_seed(torch.initial_seed() if seed is None else seed)
    for name, p in model.named_parameters():
        shape = tuple(p.shape)
        if name.endswith("tok_emb.weight") or name.endswith("tok_emb.0.weight"):
            v = torch.randn(shape, generator=g)
        elif name.endswith("coord_mlp.2.weight"):
            bound = 1e-3 * math.sqrt(6.0 / (shape[0] + shape[1]))
            v = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif len(shape) == 2:
            bound = 1.0 / math.sqrt(shape[1])
            v = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif is_layernorm(name):
            v = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
        else:  # Linear bias: fan_in of the matching weight
            wname = name[: -len("bias")] + "weight"
            fan_in = dict(model.named_parameters())[wname].shape[1]
            v = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        p.copy_(v.to(p.device))
    model.engine.refresh_shadows()


def injection_prefix(tokenizer, fill_in_from: str, do_suffix: bool):
    """The prompt of the [UNK]-injection generators: [CLIP][UNK]<fill_in_from> (+ [SUFFIX][MIDDLE]) as token ids, from the
    tokenizer's text, or from its *_token attributes for a tokenizer without tokenize_text"""
    if hasattr(tokenizer, "tokenize_text"):
        return tokenizer.tokenize_text("[CLIP][UNK]" + fill_in_from + ("[SUFFIX][MIDDLE]" if do_suffix else ""), pad=False)
    names = ["clip_token", "unk_token", "smiles_token" if fill_in_from == "[SMILES]" else "graph_token"]
    names += ["suffix_token", "middle_token"] if do_suffix else []
    return [int(getattr(tokenizer, n)) for n in names]


def beam_decodings(engine, tokenizer, prefix, h_token, beams, keep_special, return_tokens, length_penalty, grammar=None):
    """Engine.beam_search from `prefix` with h_token [G, C] in the [UNK] slot, as per-embedding lists of (smiles, log_likelihood), best
    first (the token lists themselves for a tokenizer that cannot decode); return_tokens: (those, the hypotheses' token lists: the
    prompt and the generated tokens up to and with [STOP]).  grammar: Engine.beam_search's (the scores are then renormalised over the
    admitted tokens)."""
    tokens, scores, lengths, _ = engine.beam_search(prefix=prefix, stop_token=tokenizer.stop_token, pad_token=tokenizer.pad_token,
                                                    beams=beams, inj_token=tokenizer.unk_token, inj_payload=h_token,
                                                    length_penalty=length_penalty, grammar=grammar)
    tokens, scores, lengths = tokens.tolist(), scores.tolist(), lengths.tolist()
    m = len(prefix)
    rows = [[hyp[:m + n] for hyp, n in zip(tg, ng)] for tg, ng in zip(tokens, lengths)]
    text = (lambda t: tokenizer.decode(t, special=keep_special)) if hasattr(tokenizer, "decode") else (lambda t: t)
    out = [[(text(t), float(sc)) for t, sc in zip(rg, sg)] for rg, sg in zip(rows, scores)]
    return (out, rows) if return_tokens else out


def attach_xformer_logits(xformer: nn.Module, engine: Engine):
    """RotarySmilesTransformer.forward(idx) and .forward_with_replacement(idx, injection, tokenizer, inject_token) (smiles_xformer.py:375-382,
    426-454; simple_coati2/smiles_xformer.py:388, 439) on `xformer`, so that xformer(idx) works as well: the decoder pass over the padded
    [B, T] rows and the lm_head as f32 logits [B, T, n_tok] (coati_engine_decoder_logits).  injection [B, C]: row b's vector at every
    inject_token position of row b.  The engine injects at its [UNK] id only: another inject_token raises NotImplementedError."""
    def forward(idx):
        return engine.decoder_logits(idx.to(engine.device, torch.long).contiguous())

    def forward_with_replacement(idx, injection, tokenizer, inject_token="[UNK]"):
        inj_id = int(tokenizer.vocab[inject_token])
        if inj_id != engine.cfg.unk_token:
            raise NotImplementedError(f"forward_with_replacement: the engine injects at its [UNK] id {engine.cfg.unk_token}, not at "
                                      f"{inject_token!r} ({inj_id})")
        idx = idx.to(engine.device, torch.long).contiguous()
        return engine.decoder_logits(idx, injection)

    object.__setattr__(xformer, "forward", forward)
    object.__setattr__(xformer, "forward_with_replacement", forward_with_replacement)


def _trim_columns(t, n):
    return t[:, :n].contiguous()


def score_host_rows(engine, tokens, y_next, h=None, raw_tokens=None, differentiable=False, coati2=False):
    """Engine.score (coati2: Engine.score_coati2) on host-built rows: columns behind every row's last live position are dropped (their
    targets are -1 and, under causal attention, they change no earlier logit) and the passes run on packed rows.  differentiable (with
    h): the same call through HclipLikelihood (coati2: HcoatiLikelihood), so that the result carries the gradient w.r.t. h.  Raises
    on the error word: a row without [STOP], a packed-row mismatch."""
    from ...synthetic import packed_lengths
    dev = engine.device
    l_raw, l_tok = packed_lengths(raw_tokens if raw_tokens is not None else tokens, tokens, y_next, pad=engine.cfg.pad_token)   # (l_raw unused without raw_tokens)
    T2 = max(int(l_tok.max()), 1)
    tokens, y_next = _trim_columns(tokens, T2).to(dev, torch.long), _trim_columns(y_next, T2).to(dev, torch.long)
    rows = (int(l_raw.sum()), int(l_tok.sum()))
    if raw_tokens is not None:
        raw_tokens = _trim_columns(raw_tokens, max(int(l_raw.max()), 1)).to(dev, torch.long)
    if differentiable:
        from ..autograd_funs.likelihood import HclipLikelihood, HcoatiLikelihood
        nll = (HcoatiLikelihood if coati2 else HclipLikelihood).apply(h, engine, tokens, y_next, rows)
    elif coati2:
        nll = engine.score_coati2(tokens, y_next, h_coati=h, raw_tokens=raw_tokens, rows=rows)
    else:
        nll = engine.score(tokens, y_next, h_clip=h, raw_tokens=raw_tokens, rows=rows)
    err = int(engine.scal[6:7].view(torch.int32).item())
    if err & 1:
        raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
    if err & 2:
        raise RuntimeError("packed rows: the row counts passed to score() differ from what the device found in the tokens")
    return nll


class e3gnn_smiles_clip_e2e(nn.Module):
    """Drop-in for coati.models.encoding.clip_e2e.e3gnn_smiles_clip_e2e (clip_e2e.py:350-463, 772-845)."""

    def __init__(self, n_layer_e3gnn: int = 4, n_layer_xformer: int = 16, n_hidden_xformer: int = 128,
                 n_hidden_e3nn: int = 128, msg_cutoff_e3nn: float = 4.0, n_embd_common: int = 128, n_head: int = 8,
                 n_seq: int = 200, n_tok: int = 4, biases: bool = True, torch_emb: bool = False, residual: bool = False,
                 norm_clips: bool = True, norm_embed: bool = False, token_mlp: bool = True,
                 use_point_encoder: bool = True, old_architecture: bool = False,
                 device: torch.device = torch.device("cuda:0"), dtype: torch.dtype = torch.float):
        super().__init__()
        # every constructor flag follows the reference in both settings (clip_e2e.py:357-437, 454-463; the reference's own do_args()
        # defaults are norm_clips=False, token_mlp=False: train_coati.py:520-523).  residual + torch_emb together are refused by the
        # engine: the reference builds that model and fails in its first forward (28-wide node MLP input, H-wide features)
        if dtype not in (torch.float, torch.float32):
            raise NotImplementedError("parameters are fp32 master weights (bf16 is an internal operand format)")
        self.embed_dim = n_embd_common
        self.device = torch.device(device)
        # msg_cutoff_e3nn is accepted and ignored exactly as in the reference: e3gnn_clip never forwards it to
        # its e_gcl_sparse layers, so the effective cutoff is 5.0.
        cfg = ModelConfig(n_layer_e3gnn=n_layer_e3gnn, n_layer_xformer=n_layer_xformer, n_hidden_xformer=n_hidden_xformer,
                          n_hidden_e3nn=n_hidden_e3nn, n_embd_common=n_embd_common, n_head=n_head, n_seq=n_seq, n_tok=n_tok,
                          msg_cutoff=5.0, norm_clips=bool(norm_clips), token_mlp=bool(token_mlp),
                          use_point_encoder=bool(use_point_encoder), biases=bool(biases), norm_embed=bool(norm_embed),
                          torch_emb=bool(torch_emb), old_architecture=bool(old_architecture), residual=bool(residual))
        eng = Engine(cfg, self.device, train=True)
        object.__setattr__(self, "engine", eng)
        grads = eng.named_views("grads")
        views = eng.named_views("params")
        for name in reference_parameter_order(views):
            _attach(self, name, views[name], grads[name])
        for l in range(n_layer_xformer):   # causal-mask buffers of the reference state_dict (basic_transformer.py:117-123)
            _attach(self, f"xformer.transformer.h.{l}.attn.bias",
                    torch.tril(torch.ones(n_seq, n_seq, device=self.device)).view(1, 1, n_seq, n_seq), buffer=True)
        self.xformer.n_seq, self.xformer.n_tok, self.xformer.n_embd = n_seq, n_tok, n_hidden_xformer
        # generation entry point of the reference's RotarySmilesTransformer (smiles_xformer.py:272-351), KV-cached here
        object.__setattr__(self.xformer, "generate_top_k_with_inj_batch", eng.generate_top_k_with_inj_batch)
        # prompt completion and one-sequence generation (smiles_xformer.py:157-198, 215-270): prompt prefill + per-row prompts
        object.__setattr__(self.xformer, "generate_topk_batch", eng.generate_topk_batch)
        object.__setattr__(self.xformer, "generate_topk_with_inj", eng.generate_topk_with_inj)
        attach_xformer_logits(self.xformer, eng)
        self.point_encoder.hidden_nf = n_hidden_e3nn
        self.use_point_encoder = bool(use_point_encoder)
        if not token_mlp:
            self.point_clip_to_special_tokens = nn.Identity()   # clip_e2e.py:436-437
        else:   # point_clip_to_special_tokens(h) as in the reference: SiLU -> Linear on [B, E] rows (special_tokens_from_clip)
            object.__setattr__(self.point_clip_to_special_tokens, "forward", self.special_tokens_from_clip)
        self.clip_loss = clip_loss(eng)
        self.reset_parameters()
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.engine.refresh_shadows())
        n_blocks = sum(p.numel() for n, p in self.named_parameters() if ".transformer." in n)
        n_g = sum(p.numel() for n, p in self.named_parameters() if n.startswith("point_encoder."))
        n_x = sum(p.numel() for n, p in self.named_parameters() if n.startswith("xformer."))
        print("number of parameters: %.2fM" % (n_blocks / 1e6,))
        print(f"number of parameters Total: {n_g/1e6:.2f}M xformer: {n_x/1e6:.2f}M Total: {(n_g+n_x)/1e6:.2f}M ")

    @torch.no_grad()
    def reset_parameters(self, seed: int = None):
        """torch.nn default initialisers for every layer type on the path (torch_default_init; coord_mlp.2: xavier-uniform gain 1e-3)."""
        torch_default_init(self, seed, lambda name: ".ln_" in name or ".norm_embed." in name or ".tok_emb.1." in name or name.endswith("_to_clip.0.weight")
                           or name.endswith("_to_clip.0.bias"))

    # ---- reference API ------------------------------------------------------------------------------------------
    def _tok(self, t):
        return t.to(self.device, torch.long).contiguous()

    def forward_dist(self, raw_tokens, augmented_tokens, atoms, coords, tokenizer, p_clip_emb_smi: float = 0.4,
                     use_point: torch.Tensor = None, return_logits: bool = True):
        """clip_e2e.py:772-814.  Returns (h_e3gnn, h_smiles, logits, bad_rows).  `use_point` overrides the RNG draw."""
        eng = self.engine
        self._sync_tokens(tokenizer)
        B = atoms.shape[0]
        if use_point is None:
            use_point = torch.rand((B,), device=self.device) > p_clip_emb_smi
        h_e, h_s, bad = eng.forward(self._tok(raw_tokens), self._tok(augmented_tokens), self._tok(atoms),
                                    coords.to(self.device), use_point.to(self.device), y_next=None, train=False)
        err = int(eng.scal[6:7].view(torch.int32).item())
        if err & 1:
            raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
        logits = eng.logits() if return_logits else None
        return h_e, h_s, logits, bad.bool()

    def forward(self, raw_tokens, augmented_tokens, atoms, coords, tokenizer, p_clip_emb_smi: float = 0.4):
        """clip_e2e.py:816-845: as forward_dist, fourth output = clip loss."""
        h_e, h_s, logits, bad = self.forward_dist(raw_tokens, augmented_tokens, atoms, coords, tokenizer, p_clip_emb_smi)
        return h_e, h_s, logits, self.clip_loss(h_s, h_e, bad)

    def encode_tokens(self, token_indices, tokenizer):
        """clip_e2e.py:448-452: smiles_to_clip(xformer.encode(tokens)) -- the encoder pass alone."""
        self._sync_tokens(tokenizer)
        h_s, _ = self.engine.encode(raw_tokens=self._tok(token_indices))
        if int(self.engine.scal[6:7].view(torch.int32).item()) & 1:
            raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
        return h_s

    def encode_points(self, atoms, coords):
        """clip_e2e.py:454-463: point_to_clip(point_encoder(atoms, coords)) -- the point encoder alone."""
        _, h_e = self.engine.encode(atoms=self._tok(atoms), coords=coords)
        return h_e

    def special_tokens_from_clip(self, h_clip):
        """point_clip_to_special_tokens = SiLU -> Linear (clip_e2e.py:432-435) on [B, E] embeddings (HIP silu + f32 GEMM)."""
        from ... import _lib, ops
        h = h_clip.to(self.device, torch.float32).contiguous()
        if not self.engine.cfg.token_mlp:
            return h          # nn.Identity (clip_e2e.py:436-437)
        a = torch.empty_like(h)
        _lib.call("coati_silu", ops.ptr(h), ops.ptr(a), h.numel(), ops.stream())
        lin = self.point_clip_to_special_tokens._modules["1"]
        return ops.sgemm(a, lin.weight.detach(), trans_b=True, bias=lin.bias.detach())

    @torch.no_grad()
    def hclip_to_2d_batch(self, h_clip, tokenizer, fill_in_from: str = "[SMILES]", noise_scale: float = 0.0,
                          inv_temp: float = 2, k: int = 100, do_suffix=False, keep_special: bool = False,
                          return_tokens: bool = False, generator=None, slots=None, grammar=None):
        """clip_e2e.py:544-588: decode a batch of clip embeddings into token sequences (and SMILES when the tokenizer
        can decode).  Prefix "[CLIP][UNK]" + fill_in_from (+ "[SUFFIX][MIDDLE]"), the [UNK] slot carries the
        special-token embedding of h_clip; generation = top-k sampling on the KV-cached decode path.
        slots: None = one aligned batch of all rows; a number = Engine.generate_stream on that many cache slots (rows that have
        stopped hand their slot to the next embedding; the draws of a seed differ from the aligned path's).
        grammar (coati_amd.grammar.SmilesGrammar.from_tokenizer(tokenizer)): syntax-constrained decoding -- every string has its
        parentheses, ring digits and bracket atoms closed and ends in a drawn [STOP]; aligned path only (not with slots)."""
        self._sync_tokens(tokenizer)
        assert fill_in_from in ("[SMILES]", "[GRAPH]")
        if noise_scale > 0:
            h_clip = h_clip + noise_scale * torch.randn_like(h_clip)
        h_token = self.special_tokens_from_clip(h_clip)
        prefix = injection_prefix(tokenizer, fill_in_from, do_suffix)
        if slots is None:
            generation = self.engine.generate_top_k_with_inj_batch(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp,
                                                                   k=k, pad_token=tokenizer.pad_token, inj_token=tokenizer.unk_token,
                                                                   inj_payload=h_token, generator=generator, grammar=grammar)
        else:
            generation = self.engine.generate_stream(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp, k=k,
                                                     pad_token=tokenizer.pad_token, inj_token=tokenizer.unk_token, inj_payload=h_token,
                                                     slots=int(slots), generator=generator, grammar=grammar)
        if hasattr(tokenizer, "decode"):
            smiles_list = [tokenizer.decode(t, special=keep_special) for t in generation]
        else:
            smiles_list = generation
        return (smiles_list, generation) if return_tokens else smiles_list

    @torch.no_grad()
    def points_to_2d_batch(self, atom_batch, coords_batch, tokenizer, fill_in_from: str = "[SMILES]", noise_scale: float = 0.0,
                           do_suffix: bool = False, inv_temp: float = 2, k=100, keep_special=False, generator=None, slots=None,
                           grammar=None):
        """clip_e2e.py:590-632: encode_points, then the hclip_to_2d_batch flow (noise added out of place; slots, grammar as there)."""
        h_clip = self.encode_points(atom_batch, coords_batch)
        return self.hclip_to_2d_batch(h_clip, tokenizer, fill_in_from=fill_in_from, noise_scale=noise_scale, inv_temp=inv_temp, k=k,
                                      do_suffix=do_suffix, keep_special=keep_special, generator=generator, slots=slots, grammar=grammar)

    @torch.no_grad()
    def hclip_to_2d_beam(self, h_clip, tokenizer, beams: int = 4, fill_in_from: str = "[SMILES]", do_suffix: bool = False,
                         keep_special: bool = False, return_tokens: bool = False, length_penalty: float = 0.0, grammar=None):
        """The `beams` most likely decodings of every clip embedding of h_clip [G, E], by beam search (Engine.beam_search) from the
        prompt of hclip_to_2d_batch: per embedding a list of (smiles, log_likelihood), best first -- the log-likelihood is the sum of
        the generated tokens' log-probabilities, [STOP] included.  return_tokens=True: also the hypotheses' token lists, per embedding
        (the prompt, the generated tokens up to and with [STOP]).  No reference counterpart (the reference only samples).
        grammar: see Engine.beam_search."""
        self._sync_tokens(tokenizer)
        assert fill_in_from in ("[SMILES]", "[GRAPH]")
        h_token = self.special_tokens_from_clip(h_clip)
        prefix = injection_prefix(tokenizer, fill_in_from, do_suffix)
        return beam_decodings(self.engine, tokenizer, prefix, h_token, beams, keep_special, return_tokens, length_penalty, grammar)

    @torch.no_grad()
    def points_to_2d_beam(self, atoms, coords, tokenizer, beams: int = 4, fill_in_from: str = "[SMILES]", do_suffix: bool = False,
                          keep_special: bool = False, return_tokens: bool = False, length_penalty: float = 0.0, grammar=None):
        """encode_points, then hclip_to_2d_beam."""
        return self.hclip_to_2d_beam(self.encode_points(atoms, coords), tokenizer, beams=beams, fill_in_from=fill_in_from,
                                     do_suffix=do_suffix, keep_special=keep_special, return_tokens=return_tokens,
                                     length_penalty=length_penalty, grammar=grammar)

    def _to_2d_one(self, h_clip, tokenizer, fill_in_from, noise_scale, suffix, inv_temp, k, generator, grammar=None):
        """hclip_to_2d / points_to_2d: the special token of h_clip injected as the reference does it, h_token[0] -- the first row of a
        [B, E] input, and for a 1-D [E] input its first CHANNEL, a scalar that the reference's assignment spreads over all C."""
        self._sync_tokens(tokenizer)
        assert fill_in_from in ("[SMILES]", "[GRAPH]")
        h = h_clip.to(self.device, torch.float32)
        if noise_scale > 0:
            h = h + noise_scale * torch.randn_like(h)
        h_token = self.special_tokens_from_clip(h if h.dim() == 2 else h.reshape(1, -1))
        payload = h_token[0] if h.dim() == 2 else h_token[0, 0]
        prefix = tokenizer.tokenize_text("[CLIP][UNK]" + fill_in_from + suffix, pad=False)
        generation = self.engine.generate_topk_with_inj(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp, k=k,
                                                        inj_token=tokenizer.unk_token, inj_payload=payload, generator=generator,
                                                        grammar=grammar)
        return tokenizer.decode(generation, special=False) if fill_in_from == "[SMILES]" else tokenizer.decode(generation)

    @torch.no_grad()
    def points_to_2d(self, atoms, coords, tokenizer, fill_in_from: str = "[SMILES]", noise_scale: float = 0.0, inv_temp: float = 2,
                     k: int = 100, generator=None, grammar=None):
        """clip_e2e.py:465-501: one molecule's atoms / coords -> SMILES (prefix [CLIP][UNK]<fill_in_from>[SUFFIX][MIDDLE]).
        grammar: as in hclip_to_2d_batch."""
        h_clip = self.encode_points(atoms, coords)
        return self._to_2d_one(h_clip, tokenizer, fill_in_from, noise_scale, "[SUFFIX][MIDDLE]", inv_temp, k, generator, grammar)

    @torch.no_grad()
    def hclip_to_2d(self, h_clip, tokenizer, fill_in_from: str = "[SMILES]", noise_scale: float = 0.0, do_suffix: bool = False,
                    inv_temp: float = 2, k: int = 100, generator=None, grammar=None):
        """clip_e2e.py:503-542: one embedding ([1, E] or [E]) -> SMILES (prefix [CLIP][UNK]<fill_in_from>, + [SUFFIX][MIDDLE]).
        grammar: as in hclip_to_2d_batch."""
        return self._to_2d_one(h_clip, tokenizer, fill_in_from, noise_scale, "[SUFFIX][MIDDLE]" if do_suffix else "", inv_temp, k,
                               generator, grammar)

    @torch.no_grad()
    def complete_batch(self, prefixes: List[str], tokenizer, inv_temp: float = 2, k: int = 100, keep_special: bool = False,
                       de_fim: bool = True, generator=None, grammar=None):
        """clip_e2e.py:744-770: continue text prompts of different lengths (e.g. fill-in-middle [SMILES]..[SUFFIX]..[MIDDLE]);
        no injection.  Returns the decoded strings.  grammar: the prompts' tokens advance the automaton, the completion closes what
        they opened (Engine.generate_topk_batch)."""
        self._sync_tokens(tokenizer)
        tokens = [tokenizer.tokenize_text(p, pad=False) for p in prefixes]
        generation = self.engine.generate_topk_batch(prefix=tokens, stop_token=tokenizer.stop_token, pad_token=tokenizer.pad_token,
                                                     inv_temp=inv_temp, k=k, generator=generator, grammar=grammar)
        return [tokenizer.decode(t, special=keep_special, de_fim=de_fim) for t in generation]

    def _score(self, tokens, y_next, h_clip=None, raw_tokens=None, differentiable=False):
        """score_host_rows on this model's engine (Engine.score / HclipLikelihood)"""
        return score_host_rows(self.engine, tokens, y_next, h_clip, raw_tokens, differentiable)

    def hclip_and_tokens_to_likelihood(self, hclip: torch.Tensor, smiles, tokenizer) -> torch.Tensor:
        """clip_e2e.py:634-665: summed NLL of [CLIP][UNK][SMILES][SUFFIX][MIDDLE]<smiles>[STOP] with hclip's special token at [UNK].
        hclip [E] + one SMILES string -> [1] (the reference's form); hclip [B, E] + a list of B strings -> [B] in one engine call.

        As in the reference the result is differentiable w.r.t. hclip: with grad mode on and hclip.requires_grad it carries a grad_fn
        (HclipLikelihood) and .backward() leaves d NLL / d hclip in hclip.grad.  The gradient reaches hclip ONLY: the model's parameters
        are constants of this call (the engine owns them as flat buffers outside autograd).  Otherwise nothing is recorded and the
        values are those of the plain scoring call, bit for bit."""
        self._sync_tokens(tokenizer)
        single = isinstance(smiles, str)
        want_grad = torch.is_grad_enabled() and hclip.requires_grad
        with torch.set_grad_enabled(want_grad):
            h = hclip.to(self.device, torch.float32)
            if single:
                assert h.dim() == 1, "one SMILES string goes with one embedding [E]"
                smiles, h = [smiles], h.unsqueeze(0)
            assert h.dim() == 2 and h.shape[0] == len(smiles), "hclip [B, E] needs a list of B SMILES strings"
            tokens, y_next = hclip_likelihood_tokens(list(smiles), tokenizer)
            return self._score(tokens, y_next, h_clip=h.contiguous(), differentiable=want_grad)

    @torch.no_grad()
    def batch_smiles_to_s2s_likelihood(self, smiles: List[str], tokenizer):
        """clip_e2e.py:667-742: SMILES -> hclip (encode_tokens of [SMILES]<smi>[STOP]) -> SMILES round-trip NLL per molecule.
        Returns (nll [n_ok], mask [len(smiles)]): rows that do not tokenize into n_seq - 5 positions are dropped and False in mask."""
        self._sync_tokens(tokenizer)
        raw_tokens, tokens, y_next, mask = s2s_likelihood_tokens(smiles, tokenizer)
        return self._score(tokens, y_next, raw_tokens=raw_tokens), mask.to(self.device)

    def _sync_tokens(self, tokenizer):
        if tokenizer is None:
            return
        c = self.engine.cfg
        stop, unk = getattr(tokenizer, "stop_token", c.stop_token), tokenizer.vocab["[UNK]"] if hasattr(tokenizer, "vocab") else c.unk_token
        if (stop, unk) != (c.stop_token, c.unk_token):
            raise NotImplementedError("tokenizer special ids differ from the engine's (stop/unk); rebuild the model with them")


def _formula_text(atoms_row) -> str:
    """"[FORMULA][ELM6][NUM6]..." from the element counts of one molecule (clip_e2e.py:126-141); empty when an element
    occurs 150 times or more."""
    import numpy as np
    z = np.asarray(atoms_row).astype(int)
    counts = np.bincount(z[z > 0])
    if not (counts < 150).all():
        return ""
    return "[FORMULA]" + "".join(f"[ELM{el}][NUM{n}]" for el, n in enumerate(counts) if n > 0)


def _two_cut_points(rng, lo, hi):
    """two distinct sorted positions in [lo, hi], redrawn as a pair until they differ (clip_e2e.py:158-165, 198-202)"""
    a = b = 1
    while a == b:
        a, b = sorted([rng.randint(lo, hi), rng.randint(lo, hi)])
    return a, b


def clip_ar_xform(batch: Dict[str, Any], tokenizer, p_dataset: float = 0.2, p_formula: float = 0.2, p_fim: float = 0.0,
                  p_graph: float = 0.0, p_clip: float = 0.9, p_clip_cut: float = 0.3, p_randsmiles: float = 0.0,
                  dtype: torch.dtype = torch.float, device: torch.device = torch.device("cpu"), coord_noise: bool = False,
                  canon_smiles=None, permute_smiles=None, adj_mat_to_tokens=None, rng=None):
    """coati.models.encoding.clip_e2e.clip_ar_xform (clip_e2e.py:50-330) with the reference's signature: per-row
    representation choice ([SET] / [FORMULA] / graph prefixes in shuffled order), tokenisation (C++ trie tokenizer),
    the [CLIP][UNK] prefix with probability p_clip -- with probability p_clip_cut in its fill-in-the-middle form
    [CLIP][UNK] head [SUFFIX] tail [MIDDLE] middle [STOP] --, else plain fill-in-the-middle ([PREFIX] ...) with
    probability p_fim, the raw [SMILES]...[STOP] row for the encoder pass (optionally of a permuted SMILES), oversize
    fallback to the un-augmented row, failure rows (all-[PAD] `tokens`, [STOP][PAD]... `raw_tokens`), then the
    tensorisation tail (tensorize_batch below).

    The draws come from `rng` (default: the `random` module) in the reference's order, so a seeded run reproduces the
    reference's batch.  rdkit is not a dependency: `canon_smiles` (Chem.CanonSmiles in the reference), `permute_smiles`
    and `adj_mat_to_tokens` are injected callables; canonicalisation defaults to the identity, the other two are needed
    only when p_randsmiles > 0 / a graph representation is drawn."""
    import random as _random
    import numpy as np
    rng = rng or _random
    for need in ("smiles", "source_collection", "atoms", "coords"):
        assert need in batch
    canon = canon_smiles or (lambda s: s)
    n_seq = tokenizer.n_seq
    fixed = {}                      # the sentinel strings are encoded once per call, not once per row

    def enc(text):
        if text in fixed:
            return list(fixed[text])
        ids = tokenizer.tokenize_text(text, pad=False, range_check=False)
        if text in ("[CLIP][UNK]", "[SUFFIX]", "[MIDDLE]", "[PREFIX]"):
            fixed[text] = list(ids)
        return ids

    tok_rows, raw_rows = [], []

    def fail_row():
        r = np.zeros(n_seq, dtype=np.int64)
        r[0] = tokenizer.stop_token
        raw_rows.append(r)
        tok_rows.append(np.zeros(n_seq, dtype=np.int64))

    def padded(ids):
        r = np.zeros(n_seq, dtype=np.int64)
        r[: len(ids)] = ids
        return r

    for k, smi_in in enumerate(batch["smiles"]):
        smi = canon(smi_in)
        try:
            # -- which representations, in which order (three draws, then one shuffle) --
            reps = ["smiles"]
            if rng.random() < p_dataset and "[" + batch["source_collection"][k] + "]" in tokenizer.special_tokens:
                reps.append("set")
            if rng.random() < p_formula:
                reps.append("formula")
            if rng.random() < p_graph and "adj_mat" in batch and "adj_mat_atoms" in batch:
                reps.append("graph")
            rng.shuffle(reps)
            parts = {"set": lambda: "[SET][" + batch["source_collection"][k] + "]", "smiles": lambda: "[SMILES]" + smi,
                     "formula": lambda: _formula_text(batch["atoms"][k]),
                     "graph": lambda: adj_mat_to_tokens(batch["adj_mat"][k], batch["adj_mat_atoms"][k])}
            ids = enc("".join(parts[r]() for r in reps) + "[STOP]")
            # -- [CLIP][UNK] prefix / fill-in-the-middle --
            if rng.random() < p_clip and len(ids) > 3:
                if rng.random() < p_clip_cut:
                    stop = ids.pop()
                    m, sfx = _two_cut_points(rng, 2, len(ids))      # never inside the first two tokens
                    ids = enc("[CLIP][UNK]") + ids[:m] + enc("[SUFFIX]") + ids[sfx:] + enc("[MIDDLE]") + ids[m:sfx] + [stop]
                else:
                    ids = enc("[CLIP][UNK]") + ids
            elif rng.random() < p_fim and len(ids) > 4:
                stop = ids.pop()
                m, sfx = _two_cut_points(rng, 1, len(ids))
                ids = enc("[PREFIX]") + ids[:m] + enc("[SUFFIX]") + ids[sfx:] + enc("[MIDDLE]") + ids[m:sfx] + [stop]
            # -- the encoder pass's row --
            plain = None
            if rng.random() < p_randsmiles:
                if permute_smiles is None:
                    raise RuntimeError("p_randsmiles > 0 needs a permute_smiles callable (rdkit is not a dependency)")
                raw_ids = enc("[SMILES]" + permute_smiles(smi) + "[STOP]")
                plain = enc("[SMILES]" + smi + "[STOP]")
            else:
                raw_ids = enc("[SMILES]" + smi + "[STOP]")
                plain = raw_ids
            if len(ids) <= n_seq and len(raw_ids) <= n_seq:
                tok_rows.append(padded(ids)); raw_rows.append(padded(raw_ids))
            elif len(raw_ids) <= n_seq and len(plain) <= n_seq:
                tok_rows.append(padded(plain)); raw_rows.append(padded(raw_ids))      # oversize: fall back to the plain row
            else:
                fail_row()
                print("Too much seq data.", "[SMILES]" + smi + "[STOP]", len(raw_ids))
        except Exception as ex:
            print("Tokenize failure:", smi, " Except:", ex)
            fail_row()
    out = batch
    out["tokens"] = torch.from_numpy(np.stack(tok_rows, 0)).to(device)
    out["raw_tokens"] = torch.from_numpy(np.stack(raw_rows, 0)).to(device)
    return tensorize_batch(out, tokenizer, dtype=dtype, device=device, coord_noise=coord_noise, inplace=True)


def tensorize_batch(batch: Dict[str, Any], tokenizer, dtype=torch.float, device="cpu", coord_noise=False, inplace=False):
    """The tensorisation tail of clip_ar_xform (clip_e2e.py:288-330): given stacked `tokens` / `raw_tokens`
    ([B, n_seq] long) plus atoms/coords arrays, move to `device`, truncate columns to the longest row, build y_next
    with the five masked special ids.  (`batch_pipe.device_tail` is the same tail as two HIP kernels.)"""
    out = batch if inplace else dict(batch)
    for col in ("tokens", "atoms", "raw_tokens"):
        if not isinstance(out[col], torch.Tensor):
            out[col] = torch.tensor(out[col], requires_grad=False)
    if not out["tokens"].is_cuda and not out["raw_tokens"].is_cuda and tokenizer.pad_token == 0:
        # packed-row counts (coati_hip.h, coati_engine_forward rows1 / rows2) while the tokens are still on the host: the
        # engine then skips the padding the reference computes (a target y_next[t] != -1 implies a token at t + 1, so the
        # token matrix alone gives the counts)
        from ...synthetic import packed_rows
        out["rows"] = torch.tensor(packed_rows(out["raw_tokens"], out["tokens"]), dtype=torch.int64)
    for col in ("tokens", "atoms", "raw_tokens"):
        out[col] = out[col].to(device, torch.long)
    if not isinstance(out["coords"], torch.Tensor):
        out["coords"] = torch.tensor(out["coords"], requires_grad=False)
    out["coords"] = out["coords"].to(device, dtype)
    if out["atoms"].shape[0] < 1:
        raise Exception("empty batch")
    if coord_noise:
        out["coords"] = out["coords"] + torch.normal(torch.zeros_like(out["coords"]), 0.05 * torch.ones_like(out["coords"]))
    out["tokens"] = out["tokens"][:, : int((out["tokens"].sum(0) > 0).sum())]
    out["raw_tokens"] = out["raw_tokens"][:, : int((out["raw_tokens"].sum(0) > 0).sum())]
    y = torch.zeros_like(out["tokens"])
    y[:, : out["tokens"].shape[1] - 1] = out["tokens"][:, 1:].clone()
    for t in (tokenizer.clip_token, tokenizer.pad_token, tokenizer.unk_token, tokenizer.suffix_token, tokenizer.middle_token):
        y[y == t] = -1
    out["y_next"] = y
    return out
