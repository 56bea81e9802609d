"""COATI2's model (simple_coati2/transformer_only.py:19-200) with the reference's constructor, state_dict names and methods;
trainable=True adds the training step the reference does not have (Engine.train_step on a COATI2 layout: AR loss, clip-norm, AdamW).
The transformer, both heads and generation run in libcoati_hip.so through coati_amd.engine.Engine; this file adapts the
calling convention.  SwiGLU / SwiGLUResNet are the reference's torch modules, kept for code that builds them directly."""
import torch
import torch.nn as nn

from ...engine import Engine, ModelConfig
from ..encoding.clip_e2e import (_attach, attach_xformer_logits, beam_decodings, hcoati_likelihood_tokens, injection_prefix, reference_parameter_order,
                                 s2s_hcoati_likelihood_tokens, score_host_rows, torch_default_init)


class SwiGLUResNet(nn.Module):
    """transformer_only.py:19-36: LayerNorm -> Dropout -> Linear(d_in, 2 d_out) -> SwiGLU -> Linear(d_out, d_out), + x"""

    def __init__(self, d_in, d_out, dropout=0.0):
        super().__init__()
        self.net = nn.Sequential(nn.LayerNorm(d_in), nn.Dropout(p=dropout), nn.Linear(d_in, 2 * d_out), SwiGLU(), nn.Linear(d_out, d_out))

    def forward(self, x):
        return self.net(x) + x


class SwiGLU(nn.Module):
    """transformer_only.py:38-42: x, gate = x.chunk(2, -1); silu(gate) * x, as the HIP kernel coati_swiglu on device f32 tensors."""

    def forward(self, x):
        from ... import ops
        return ops.swiglu(x.reshape(-1, x.shape[-1]).contiguous()).view(*x.shape[:-1], x.shape[-1] // 2)


def coati2_parameter_order(names):
    """The reference's parameter order (transformer_only.py:83-104): the xformer (as COATI1's, reference_parameter_order), then
    smiles_to_coati and coati_to_token, whose entries the engine's table lists in module order already."""
    names = list(names)
    return reference_parameter_order([n for n in names if n.startswith("xformer.")]) + [n for n in names if not n.startswith("xformer.")]


def _is_layernorm(name):
    return ".ln_" in name or name.endswith("_to_coati.0.weight") or name.endswith("_to_coati.0.bias") or ".net.0." in name


class COATI_Smiles_Inference(nn.Module):
    """Drop-in for coati.models.simple_coati2.transformer_only.COATI_Smiles_Inference.  No dropout (mlp_dropout is recorded), and the
    model's special ids (default: the coati2_12_12 vocabulary's [PAD] / [STOP] / [UNK]) must be the tokenizer's.
    trainable=False (default): a forward-only engine -- no gradient or Adam buffers, every step entry refuses.  trainable=True: the
    engine is built with train=True, every parameter carries its slice of the gradient buffer as .grad (as e3gnn_smiles_clip_e2e),
    model.engine.train_step(batch, None, lr, do_clip=False) runs a step and forward() returns (h_coati, logits); mlp_dropout > 0 raises
    NotImplementedError there (a training step with dropout is not implemented)."""

    def __init__(self, n_layer_xformer=16, n_hidden_xformer=256, embed_dim=256, n_head=16, n_seq=80, mlp_dropout=0.0,
                 enc_to_coati="linear", n_direct_clr=64, n_tok=4, biases=True, device=torch.device("cuda:0"), dtype=torch.float, *,
                 pad_token: int = 31, stop_token: int = 40, unk_token: int = 44, trainable: bool = False):
        super().__init__()
        if trainable and mlp_dropout > 0:
            raise NotImplementedError(f"trainable=True with mlp_dropout={mlp_dropout}: the training step has no dropout")
        if dtype not in (torch.float, torch.float32):
            raise NotImplementedError("parameters are fp32 (bf16 is an internal operand format)")
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError(f"COATI_Smiles_Inference runs on the HIP engine: device must be a GPU, not {device}")
        self.embed_dim = embed_dim
        self.enc_to_coati = enc_to_coati
        self.n_direct_clr = n_direct_clr
        self.mlp_dropout = mlp_dropout
        self.device = device
        self.trainable = bool(trainable)
        # the constructor arguments a checkpoint document records (save_coati2)
        self.model_kwargs = dict(n_layer_xformer=n_layer_xformer, n_hidden_xformer=n_hidden_xformer, embed_dim=embed_dim, n_head=n_head, n_seq=n_seq,
                                 mlp_dropout=mlp_dropout, enc_to_coati=enc_to_coati, n_direct_clr=n_direct_clr, n_tok=n_tok, biases=biases)
        cfg = ModelConfig(n_layer_xformer=n_layer_xformer, n_layer_e3gnn=0, n_hidden_xformer=n_hidden_xformer, n_hidden_e3nn=n_hidden_xformer,
                          n_embd_common=embed_dim, n_head=n_head, n_seq=n_seq, n_tok=n_tok, pad_token=int(pad_token), stop_token=int(stop_token),
                          unk_token=int(unk_token), use_point_encoder=False, biases=bool(biases), enc_to_coati=enc_to_coati)
        eng = Engine(cfg, device, train=self.trainable)
        object.__setattr__(self, "engine", eng)
        views = eng.named_views("params")
        grads = eng.named_views("grads") if self.trainable else {}
        for name in coati2_parameter_order(views):
            _attach(self, name, views[name], grads.get(name))
        for l in range(n_layer_xformer):   # causal-mask buffers of the reference state_dict (basic_transformer.py:117-123)
            _attach(self, f"xformer.transformer.h.{l}.attn.bias",
                    torch.tril(torch.ones(n_seq, n_seq, device=device)).view(1, 1, n_seq, n_seq), buffer=True)
        self.xformer.n_seq, self.xformer.n_tok, self.xformer.n_embd = n_seq, n_tok, n_hidden_xformer
        # generation entry points of the reference's RotarySmilesTransformer (smiles_xformer.py), KV-cached here
        object.__setattr__(self.xformer, "generate_top_k_with_inj_batch", eng.generate_top_k_with_inj_batch)
        object.__setattr__(self.xformer, "generate_topk_batch", eng.generate_topk_batch)
        object.__setattr__(self.xformer, "generate_topk_with_inj", eng.generate_topk_with_inj)
        # xformer(idx) / xformer.forward_with_replacement(idx, injection, tokenizer): f32 logits of the padded rows
        attach_xformer_logits(self.xformer, eng)
        # model.coati_to_token(h) as in the reference: SwiGLUResNet(E, E) on [B, E] rows (HIP LayerNorm, exact-f32 products, SwiGLU kernel)
        object.__setattr__(self.coati_to_token, "forward", eng.token_head)
        self.reset_parameters()
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.engine.refresh_shadows())
        n_x = sum(p.numel() for n, p in self.named_parameters() if n.startswith("xformer."))
        print(f"number of parameters Total: xformer: {n_x/1e6:.2f}M ")

    @torch.no_grad()
    def reset_parameters(self, seed: int = None):
        """torch.nn default initialisers (Linear: kaiming-uniform(a=sqrt 5) weight and U(+-1/sqrt(fan_in)) bias; Embedding: N(0,1);
        LayerNorm: 1/0)."""
        torch_default_init(self, seed, _is_layernorm)

    def _sync_tokens(self, tokenizer):
        if tokenizer is None:
            return
        c = self.engine.cfg
        ids = tuple(int(getattr(tokenizer, n, getattr(c, n))) for n in ("stop_token", "unk_token", "pad_token"))
        if ids != (c.stop_token, c.unk_token, c.pad_token):
            raise NotImplementedError(f"tokenizer special ids (stop/unk/pad) {ids} differ from the model's "
                                      f"{(c.stop_token, c.unk_token, c.pad_token)}; build the model with the tokenizer's ids")

    def forward(self, raw_tokens, augmented_tokens, tokenizer):
        """(h_coati [B, E], logits [B, T2, n_tok]) of the training step's forward in evaluation mode: smiles_to_coati of the encoder pass
        over raw_tokens, the decoder pass over augmented_tokens with coati_to_token(h_coati) at [UNK], the lm_head.  trainable=True only."""
        self._sync_tokens(tokenizer)
        eng = self.engine
        _, h, _ = eng.forward(raw_tokens.to(self.device, torch.long).contiguous(), augmented_tokens.to(self.device, torch.long).contiguous(),
                              y_next=None, train=False)
        if int(eng.scal[6:7].view(torch.int32).item()) & 1:
            raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
        return h, eng.logits()

    def encode_tokens(self, token_indices, tokenizer):
        """transformer_only.py:108-110: smiles_to_coati(xformer.encode(tokens)) -- the [STOP]-row embedding [B, embed_dim]."""
        assert token_indices.dim() == 2
        self._sync_tokens(tokenizer)
        h, _ = self.engine.encode(raw_tokens=token_indices.to(self.device, torch.long).contiguous())
        if int(self.engine.scal[6:7].view(torch.int32).item()) & 1:
            raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
        return h

    @torch.no_grad()
    def hcoati_to_2d(self, h_coati, tokenizer, fill_in_from="[SMILES]", noise_scale=0.0, do_suffix=False, inv_temp=2, k=100, generator=None,
                     grammar=None):
        """transformer_only.py:112-152: one embedding -> SMILES (grammar: syntax-constrained decoding, see hcoati_to_2d_batch).  The payload is h_token[0]: the first row of a [B, E] input, and for a
        1-D [E] input its first channel, a scalar the reference's assignment spreads over all C.  Noise is added out of place."""
        self._sync_tokens(tokenizer)
        assert fill_in_from == "[SMILES]" or fill_in_from == "[GRAPH]"
        h = h_coati.to(self.device, torch.float32)
        if noise_scale > 0:
            h = h + noise_scale * torch.randn_like(h)
        h_token = self.engine.token_head(h if h.dim() == 2 else h.reshape(1, -1))
        payload = h_token[0] if h.dim() == 2 else h_token[0, 0]
        prefix = injection_prefix(tokenizer, fill_in_from, do_suffix)
        generation = self.xformer.generate_topk_with_inj(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp, k=k,
                                                         inj_token=tokenizer.unk_token, inj_payload=payload, generator=generator,
                                                         grammar=grammar)
        return tokenizer.decode(generation, special=False) if fill_in_from == "[SMILES]" else tokenizer.decode(generation)

    @torch.no_grad()
    def hcoati_to_2d_batch(self, h_coati: torch.Tensor, tokenizer, fill_in_from: str = "[SMILES]", noise_scale: float = 0.0,
                           inv_temp: float = 2, k: int = 100, do_suffix=False, keep_special: bool = False, return_tokens: bool = False,
                           generator=None, slots=None, grammar=None):
        """transformer_only.py:154-200: decode [B, E] embeddings through coati_to_token at the [UNK] slot of
        [CLIP][UNK]<fill_in_from> (+ [SUFFIX][MIDDLE]); top-k sampling on the KV-cached decode path.  Noise is added out of place.
        slots: None = one aligned batch of all rows; a number = Engine.generate_stream on that many cache slots.
        grammar (coati_amd.grammar.SmilesGrammar.from_tokenizer(tokenizer)): every string has its parentheses, ring digits and bracket
        atoms closed and ends in a drawn [STOP]; aligned path only (not with slots)."""
        assert k > 1
        self._sync_tokens(tokenizer)
        h = h_coati.to(self.device, torch.float32)
        if noise_scale > 0:
            h = h + noise_scale * torch.randn_like(h)
        h_token = self.engine.token_head(h)
        prefix = injection_prefix(tokenizer, fill_in_from, do_suffix)
        assert h_token.dim() == 2
        assert h_token.shape[-1] == self.xformer.n_embd
        if slots is None:
            generation = self.xformer.generate_top_k_with_inj_batch(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp, k=k,
                                                                    pad_token=tokenizer.pad_token, inj_token=tokenizer.unk_token,
                                                                    inj_payload=h_token, generator=generator, grammar=grammar)
        else:
            generation = self.engine.generate_stream(prefix=prefix, stop_token=tokenizer.stop_token, inv_temp=inv_temp, k=k,
                                                     pad_token=tokenizer.pad_token, inj_token=tokenizer.unk_token, inj_payload=h_token,
                                                     slots=int(slots), generator=generator, grammar=grammar)
        smiles_list = [tokenizer.decode(t, special=keep_special) for t in generation]
        if return_tokens:
            return smiles_list, generation
        return smiles_list

    @torch.no_grad()
    def hcoati_to_2d_beam(self, h_coati, tokenizer, beams: int = 4, fill_in_from: str = "[SMILES]", do_suffix: bool = False,
                          keep_special: bool = False, return_tokens: bool = False, length_penalty: float = 0.0, grammar=None):
        """The `beams` most likely decodings of every embedding of h_coati [G, E], by beam search (Engine.beam_search) through
        coati_to_token at the [UNK] slot of hcoati_to_2d_batch's prompt: per embedding a list of (smiles, log_likelihood), best first;
        return_tokens=True: also the hypotheses' token lists.  No reference counterpart (the reference only samples).
        grammar: see Engine.beam_search."""
        self._sync_tokens(tokenizer)
        assert fill_in_from == "[SMILES]" or fill_in_from == "[GRAPH]"
        h_token = self.engine.token_head(h_coati.to(self.device, torch.float32))
        prefix = injection_prefix(tokenizer, fill_in_from, do_suffix)
        return beam_decodings(self.engine, tokenizer, prefix, h_token, beams, keep_special, return_tokens, length_penalty, grammar)

    def hcoati_and_tokens_to_likelihood(self, h_coati: torch.Tensor, smiles, tokenizer, do_suffix=False) -> torch.Tensor:
        """The likelihood of a SMILES string under an embedding (COATI1's hclip_and_tokens_to_likelihood, clip_e2e.py:634-665, on
        COATI2's decoding prompt): the summed NLL of [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smiles>[STOP] with coati_to_token(h_coati)
        at [UNK]; [CLIP] / [PAD] / [SMILES] / [UNK] / [SUFFIX] / [MIDDLE] targets do not count.  h_coati [E] + one string -> [1];
        h_coati [B, E] + a list of B strings -> [B] in one engine call on packed rows.

        Differentiable w.r.t. h_coati: with grad mode on and h_coati.requires_grad the result carries a grad_fn (HcoatiLikelihood) and
        .backward() leaves d NLL / d h_coati in h_coati.grad.  The gradient reaches h_coati ONLY: the model's parameters are constants
        of this call.  Otherwise nothing is recorded and the values are those of the plain scoring call, bit for bit."""
        self._sync_tokens(tokenizer)
        single = isinstance(smiles, str)
        want_grad = torch.is_grad_enabled() and h_coati.requires_grad
        with torch.set_grad_enabled(want_grad):
            h = h_coati.to(self.device, torch.float32)
            if single:
                assert h.dim() == 1, "one SMILES string goes with one embedding [E]"
                smiles, h = [smiles], h.unsqueeze(0)
            assert h.dim() == 2 and h.shape[0] == len(smiles), "h_coati [B, E] needs a list of B SMILES strings"
            tokens, y_next = hcoati_likelihood_tokens(list(smiles), tokenizer, do_suffix)
            return score_host_rows(self.engine, tokens, y_next, h=h.contiguous(), differentiable=want_grad, coati2=True)

    @torch.no_grad()
    def batch_smiles_to_s2s_likelihood(self, smiles, tokenizer, do_suffix=False):
        """SMILES -> h_coati (encode_tokens of [SMILES]<smi>[STOP]) -> SMILES round-trip NLL per molecule (COATI1's
        batch_smiles_to_s2s_likelihood, clip_e2e.py:667-742, on hcoati_and_tokens_to_likelihood's rows).  Returns (nll [n_ok],
        mask [len(smiles)]): rows that do not tokenize, or do not fit n_seq minus the prompt, are dropped and False in mask."""
        self._sync_tokens(tokenizer)
        raw_tokens, tokens, y_next, mask = s2s_hcoati_likelihood_tokens(list(smiles), tokenizer, do_suffix)
        if not bool(mask.any()):
            return torch.zeros(0, device=self.device), mask.to(self.device)
        return score_host_rows(self.engine, tokens, y_next, raw_tokens=raw_tokens, coati2=True), mask.to(self.device)
