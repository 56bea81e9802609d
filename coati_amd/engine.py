"""Host-side owner of the flat buffers + thin driver of the C engine (csrc/engine.cpp).

One `Engine` = one model replica on one GPU.  PyTorch owns every byte (parameters, gradients, AdamW state, bf16
shadows, workspace); the C library only borrows pointers while it enqueues kernels on the current stream."""
import ctypes
import math
from dataclasses import dataclass, asdict
from typing import Dict, List, Optional

import torch

from . import _lib
from .ops import ptr, stream, rope_tables
from .periodic import onehot_lut


@dataclass
class ModelConfig:
    """kwargs of the reference's e3gnn_smiles_clip_e2e (clip_e2e.py:357-378) that shape the path."""
    n_layer_e3gnn: int = 5
    n_layer_xformer: int = 16
    n_hidden_xformer: int = 256
    n_hidden_e3nn: int = 256
    n_embd_common: int = 256
    n_head: int = 16
    n_seq: int = 250
    n_tok: int = 10322
    msg_cutoff: float = 5.0
    pad_token: int = 0
    stop_token: int = 1
    unk_token: int = 7
    fp8: bool = False     # BASELINE.json configs[4]: the transformer's Linear forward / input-gradient products on MXFP8 (needs C % 128 == 0)
    # constructor flags of the reference model (clip_e2e.py:370-376): grande_closed sets all three (train_grande.py:21-35);
    # the reference's own do_args() defaults are norm_clips=False, token_mlp=False (train_coati.py:520-523)
    norm_clips: bool = True
    token_mlp: bool = True
    use_point_encoder: bool = True
    norm_embed: bool = False   # True: LayerNorm behind the token embedding (basic_transformer.py:72-76), the injection overwrites its output
    biases: bool = True   # False: c_attn / c_proj / mlpf.0 / mlpf.2 of every block without bias (basic_transformer.py:113-115, 166-168)
    torch_emb: bool = False   # True: node features = rows of nn.Embedding(84, H) instead of Linear(one-hot group / period) (e3gnn_clip.py:49-56, 113-115)
    old_architecture: bool = False   # True (with norm_clips): the two clip heads are Linear -> LayerNorm instead of LayerNorm -> Linear (clip_e2e.py:409-417)
    residual: bool = False   # True: every node MLP also sees the one-hot node features (e3gnn_clip.py:97-100, e_gcl_sparse.py:141, 282-290)
    # COATI2 (simple_coati2/transformer_only.py:43-104): "linear" / "swiglu_mlp" / "swiglu_resnet" selects smiles_to_coati, None = COATI1.
    # Engine(cfg, train=True) on a COATI2 layout trains (forward / backward / optimizer_step with atoms = coords = use_point = None: AR loss
    # only); with train=False it is inference-only (encode, token_head, decode, scoring).  The point-encoder and clip-head fields above do not apply
    enc_to_coati: Optional[str] = None


ENC_TO_COATI = {"linear": 0, "swiglu_mlp": 1, "swiglu_resnet": 2}


SCAL_AR_SUM, SCAL_AR_COUNT, SCAL_CLIP1, SCAL_CLIP2, SCAL_NVALID, SCAL_GRADNORM, SCAL_ERR = 0, 1, 2, 3, 4, 5, 6


def pack_prompts(prefix: List[List[int]], n_seq: int):
    """Host-side packing of per-row prompts for coati_topk_sample_prompt: prompt [B, n_seq] int64 (row b = prefix[b], zero-filled)
    and plen [B] int32 (the prompt lengths).  Every prompt needs 1 .. n_seq tokens."""
    B = len(prefix)
    if B == 0:
        raise ValueError("no prompts")
    prompt = torch.zeros(B, n_seq, dtype=torch.long)
    plen = torch.empty(B, dtype=torch.int32)
    for b, row in enumerate(prefix):
        n = len(row)
        if not 1 <= n <= n_seq:
            raise ValueError(f"prompt {b} has {n} tokens; 1 .. n_seq = {n_seq} fit")
        prompt[b, :n] = torch.tensor([int(t) for t in row], dtype=torch.long)
        plen[b] = n
    return prompt, plen


ERR_Z_MESSAGE = "torch_emb: an atomic number above 83 has no row in nn.Embedding(84, H) (e3gnn_clip.py:113-115)"


def _coati2_step(cfg, do_clip):
    """True on a COATI2 layout, whose step is the AR loss (+ an external dh_coati): there is no contrastive head, do_clip=True raises"""
    c2 = getattr(cfg, "enc_to_coati", None) is not None
    if c2 and do_clip:
        raise ValueError("a COATI2 engine has no contrastive head: call with do_clip=False (an external head feeds dh_coati)")
    return c2


class Engine:
    def __init__(self, cfg: ModelConfig, device="cuda:0", train=True):
        if not torch.cuda.is_available():
            raise RuntimeError("coati_amd.Engine needs an MI355X (HIP device); there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        self.l = _lib.lib()
        # by field name: the order of coati_config's fields is the header's alone
        c = _lib.CoatiConfig(n_layer_xformer=cfg.n_layer_xformer, n_layer_e3gnn=cfg.n_layer_e3gnn, n_hidden_xformer=cfg.n_hidden_xformer,
                             n_hidden_e3nn=cfg.n_hidden_e3nn, n_embd_common=cfg.n_embd_common, n_head=cfg.n_head, n_seq=cfg.n_seq,
                             n_tok=cfg.n_tok, msg_cutoff=cfg.msg_cutoff, pad_token=cfg.pad_token, stop_token=cfg.stop_token,
                             unk_token=cfg.unk_token, use_fp8=1 if cfg.fp8 else 0, norm_clips=1 if cfg.norm_clips else 0,
                             token_mlp=1 if cfg.token_mlp else 0, use_point_encoder=1 if cfg.use_point_encoder else 0,
                             biases=1 if cfg.biases else 0, norm_embed=1 if cfg.norm_embed else 0, torch_emb=1 if cfg.torch_emb else 0,
                             old_architecture=1 if cfg.old_architecture else 0, residual=1 if cfg.residual else 0)
        h = ctypes.c_void_p()
        if cfg.enc_to_coati is None:
            _lib.check(self.l.coati_engine_create(ctypes.byref(c), ctypes.byref(h)), "coati_engine_create")
        else:
            if cfg.enc_to_coati not in ENC_TO_COATI:
                raise ValueError(f"enc_to_coati must be one of {sorted(ENC_TO_COATI)}, not {cfg.enc_to_coati!r}")
            _lib.check(self.l.coati_engine_create_coati2(ctypes.byref(c), ENC_TO_COATI[cfg.enc_to_coati], ctypes.byref(h)),
                       "coati_engine_create_coati2")
        self.h = h
        self.n_params = int(self.l.coati_engine_param_elems(h))
        self.n_trainable = int(self.l.coati_engine_trainable_elems(h))
        self.n_shadow = int(self.l.coati_engine_shadow_elems(h))
        self.layout = {}
        buf = ctypes.create_string_buffer(256)
        off, rows, cols = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        for i in range(self.l.coati_engine_n_entries(h)):
            _lib.check(self.l.coati_engine_entry(h, i, buf, 256, ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols)), "entry")
            shape = (rows.value, cols.value) if cols.value > 0 else (rows.value,)
            self.layout[buf.value.decode()] = (off.value, shape)
        dev = self.device
        self.params = torch.zeros(self.n_params, device=dev, dtype=torch.float32)
        self.grads = torch.zeros(self.n_params, device=dev, dtype=torch.float32) if train else None
        self.adam_m = torch.zeros(self.n_params, device=dev, dtype=torch.float32) if train else None
        self.adam_v = torch.zeros(self.n_params, device=dev, dtype=torch.float32) if train else None
        self.shadow = torch.zeros(self.n_shadow, device=dev, dtype=torch.bfloat16)
        self.cos, self.sin = rope_tables(cfg.n_seq, cfg.n_hidden_xformer // cfg.n_head, device=dev)
        ix, iy = onehot_lut()
        self.lut_ix = torch.tensor(ix, dtype=torch.int32, device=dev)
        self.lut_iy = torch.tensor(iy, dtype=torch.int32, device=dev)
        _lib.check(self.l.coati_engine_bind(h, ptr(self.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                                            ptr(self.shadow), ptr(self.cos), ptr(self.sin), ptr(self.lut_ix),
                                            ptr(self.lut_iy)), "coati_engine_bind")
        self.shadow8 = None
        if cfg.fp8:   # MXFP8 copies of the transformer weights (e4m3 + E8M0 scales), refreshed with the bf16 shadows
            n8 = int(self.l.coati_engine_fp8_bytes(h))
            self.shadow8 = torch.zeros(n8, device=dev, dtype=torch.uint8)
            _lib.check(self.l.coati_engine_bind_fp8(h, ptr(self.shadow8), n8), "coati_engine_bind_fp8")
        self.workspace = None
        self.scal = torch.zeros(16, device=dev, dtype=torch.float32)
        self._shape = None
        self.step_count = 0
        self.last_grammar_violations = None   # bool [B] ([G, W] for beams) of the last call with grammar=: the rows that went dead
        self.last_unstopped = None            # bool [B] of the last generate_top_k_with_inj_batch: rows whose last position was overwritten with [STOP]

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.l.coati_engine_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------------------------------------
    def view(self, name, which="params"):
        off, shape = self.layout[name]
        n = math.prod(shape)
        return getattr(self, which)[off:off + n].view(*shape)

    def named_views(self, which="params"):
        return {k: self.view(k, which) for k in self.layout}

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict=True):
        missing = [k for k in self.layout if k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:5]}...")
        with torch.no_grad():
            for k in self.layout:
                if k in sd:
                    self.view(k).copy_(sd[k].to(self.device, torch.float32))
        self.refresh_shadows()
        return missing

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.named_views().items()}

    def refresh_shadows(self):
        _lib.check(self.l.coati_engine_refresh_shadows(self.h, stream()), "refresh_shadows")

    # ---- step pieces ---------------------------------------------------------------------------------------
    def _fit_workspace(self, B, T1, T2, A, Bg=None):
        """The step workspace holds what the library carves for (B, T1, T2, A) and Bg InfoNCE columns (default B): re-allocated when
        it is too small.  Returns the size asked for."""
        need = int(self.l.coati_engine_workspace_bytes(self.h, B, T1, T2, A, B if Bg is None else Bg))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = None
            self.workspace = torch.empty(need, device=self.device, dtype=torch.uint8)
        return need

    def _injection(self, injection, B):
        """an optional injection as a contiguous f32 [B, C] device tensor (or None)"""
        if injection is None:
            return None
        inj = injection.to(self.device, torch.float32).contiguous()
        assert inj.shape == (B, self.cfg.n_hidden_xformer), inj.shape
        return inj

    def _logits_rows(self, rows, want=True):
        """(buffer [rows, ld] f32, ld, its [:, :n_tok] view): ld = n_tok rounded up to 8 floats, so that the f32 rows are 16-B aligned
        for the GEMM epilogue's float4 stores.  want=False: (None, ld, None)."""
        V = self.cfg.n_tok
        ld = (V + 7) // 8 * 8
        if not want:
            return None, ld, None
        buf = torch.empty(rows, ld, device=self.device, dtype=torch.float32)
        return buf, ld, buf[:, :V]

    def _ensure_workspace(self, B, T1, T2, A):
        # Bg = columns of the InfoNCE logits: the global batch when torch.distributed is up
        world = 1
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                world = dist.get_world_size()
        except Exception:
            world = 1
        # grow-only capacities: buffers are carved for the largest shape seen so far, so that batches of different width (every batch of
        # clip_ar_xform has its own T) keep the same addresses -- cached launch tables stay valid, the workspace stops being re-sized
        # A growth event is expensive (the workspace is re-allocated -- a device-wide synchronisation --, every buffer is re-carved and
        # the cached launch tables are rebuilt: ~ 100 ms, tools/feed_e2e_probe.py), and in real training the widest row seen so far
        # keeps creeping up for hundreds of batches: widths therefore grow in steps of 32 columns (at most n_seq / 32 events per run),
        # and a trainer that knows its limits calls reserve() once up front.
        cap = getattr(self, "_cap", (0, 0, 0, 0))
        new = tuple(max(a, b) for a, b in zip(cap, (B, T1, T2, A)))
        if new != cap:
            tmax = int(self.cfg.n_seq)
            new = (new[0], min(max(tmax, new[1]), -(-new[1] // 32) * 32), min(max(tmax, new[2]), -(-new[2] // 32) * 32), new[3])
            _lib.check(self.l.coati_engine_reserve(self.h, *new), "coati_engine_reserve")
            self._cap = new
            self.growth_events = getattr(self, "growth_events", 0) + 1
        cb, c1, c2, ca = self._cap
        return self._fit_workspace(max(B, cb), max(T1, c1), max(T2, c2), max(A, ca), max(B, cb) * world)

    def reserve(self, B, T1, T2, A, headroom=0.9):
        """Carve every buffer for batches of up to B molecules, T1 / T2 token columns and A atoms now (coati_engine_reserve): later
        batches inside these limits never trigger a growth event (a growth event re-allocates the workspace -- 34 -> 42 GB when the
        width capacity goes from 128 to 160 columns at B = 1024 -- and costs ~ 1.3 s: profiles/r06_feed_e2e_probe.txt).  The buffers
        are sized for the PADDED layout of the capacity (B x T rows per pass).  Returns False, and reserves nothing, when that
        does not fit into `headroom` of the memory that is free now."""
        B, T1, T2, A = int(B), min(int(T1), int(self.cfg.n_seq)), min(int(T2), int(self.cfg.n_seq)), int(A)
        cap = getattr(self, "_cap", (0, 0, 0, 0))
        want = tuple(max(a, b) for a, b in zip(cap, (B, T1, T2, A)))
        need = int(self.l.coati_engine_workspace_bytes(self.h, *want, want[0]))
        have = self.workspace.numel() if self.workspace is not None else 0
        if need > have:
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > headroom * (free + have):
                return False
        self._ensure_workspace(B, T1, T2, A)
        return True

    def forward(self, raw_tokens, tokens, atoms=None, coords=None, use_point=None, y_next=None, train=True, rows=None, stop_after_heads=False):
        """forward_dist (+ AR loss sums when y_next is given).  Returns (h_e3gnn, h_smiles, bad_rows).
        A COATI2 engine built with train=True takes atoms = coords = use_point = None: h_smiles is h_coati (smiles_to_coati of the
        encoder pass), coati_to_token of it is injected, h_e3gnn is zeros.
        stop_after_heads: return as soon as the embeddings are final; forward_decoder() then enqueues the decoder pass + lm_head
        (the contrastive head can run on another stream in between, see train_step).
        rows = (rows1, rows2): run both transformer passes on PACKED rows -- the rows' real prefixes only, counts from
        coati_amd.synthetic.packed_rows / the batch assembler (host ints); None = the padded layout (needed by logits())."""
        B, T1 = raw_tokens.shape
        T2 = tokens.shape[1]
        if self.cfg.enc_to_coati is not None and atoms is None and coords is None and use_point is None:
            A = 1
        else:
            A = atoms.shape[1]
            coords = coords.to(torch.float32).contiguous()
            use_point = use_point.to(torch.uint8).contiguous()
        for t in (raw_tokens, tokens) + ((atoms,) if atoms is not None else ()):
            assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous()
        if y_next is not None:
            y_next = y_next.contiguous()
        self._ensure_workspace(B, T1, T2, A)
        E = self.cfg.n_embd_common
        h_e = torch.empty(B, E, device=self.device, dtype=torch.float32)
        h_s = torch.empty(B, E, device=self.device, dtype=torch.float32)
        bad = torch.empty(B, device=self.device, dtype=torch.uint8)
        self._keep = (raw_tokens, tokens, atoms, coords, use_point, y_next)  # keep inputs alive until backward
        if rows is not None:
            r1, r2 = (int(x) for x in (rows.tolist() if isinstance(rows, torch.Tensor) else rows))   # keep the tensor on the host: a device tensor costs a sync
        else:
            r1 = r2 = 0
        if r1 <= 0 or r2 <= 0:
            r1 = r2 = 0          # nothing to pack (e.g. every row failed to tokenise): padded layout
        _lib.check(self.l.coati_engine_forward(self.h, ptr(self.workspace), self.workspace.numel(), B, T1, T2, A, ptr(raw_tokens), ptr(tokens),
                                               ptr(y_next), ptr(atoms), ptr(coords), ptr(use_point), ptr(h_e), ptr(h_s),
                                               ptr(bad), ptr(self.scal), (1 if (train and self.grads is not None) else 0) | (2 if stop_after_heads else 0),
                                               r1, r2, stream()), "coati_engine_forward")
        self._shape = (B, T1, T2, A)
        self._packed = r1 > 0
        return h_e, h_s, bad

    def forward_decoder(self):
        """second half of a forward(..., stop_after_heads=True): decoder pass with the injected token, lm_head + AR cross-entropy"""
        _lib.check(self.l.coati_engine_forward_decoder(self.h, stream()), "coati_engine_forward_decoder")

    def ln_saves_xhat(self, which):
        """whether the LayerNorm-fused launches of the last forward left xhat (True) or the LayerNorm's output (False) in the saved rows of
        the encoder pass (which = 0) / decoder pass (1): the engine's per-pass, per-step decision (coati_engine_ln_saves_xhat)"""
        rc = self.l.coati_engine_ln_saves_xhat(self.h, which)
        if rc < 0:
            _lib.check(rc, "coati_engine_ln_saves_xhat")
        return bool(rc)

    def contrastive_under_decoder(self, head_fn):
        """Runs head_fn() -- the contrastive head of the step: InfoNCE / Barlow and, data-parallel, the embedding all-gather and the
        reduce-scatter around it -- on a side stream WHILE the decoder pass runs on the current one: the head only needs the
        embeddings, which are final behind the encoder pass.  Call between forward(..., stop_after_heads=True) and backward();
        enqueues the decoder pass itself.  Returns head_fn's result (tensors are safe to use on the current stream).
        (One GPU, measured round 4: 22.08 ms either way -- the head's small kernels fill the tails of the decoder pass's persistent
        kernels; the point is N > 1, where the exchange step's three collectives leave the critical path.)"""
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        self.forward_decoder()                      # first: the main stream has its work queued whatever head_fn blocks on
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            out = head_fn()
            done = torch.cuda.Event()
            done.record(self._side)
        main.wait_event(done)
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(main)               # allocated on the side stream, consumed by the backward on the main one
        return out

    def encode(self, raw_tokens=None, atoms=None, coords=None, rows=None):
        """encode_tokens / encode_points: only the requested tower runs.  Returns (h_smiles or None, h_e3gnn or None).
        rows: rows1 of the packed layout of raw_tokens (host int, coati_amd.synthetic.packed_rows): the token tower alone on packed rows
        (coati_engine_encode_packed; h_smiles as the padded encode's to bf16 rounding).  None: the padded layout."""
        if rows is not None:
            assert atoms is None and coords is None, "encode(rows=...): the packed entry runs the token tower alone"
            return self._encode_packed(raw_tokens, int(rows)), None
        assert raw_tokens is not None or atoms is not None
        B = (raw_tokens if raw_tokens is not None else atoms).shape[0]
        T1 = raw_tokens.shape[1] if raw_tokens is not None else 1
        A = atoms.shape[1] if atoms is not None else 1
        E = self.cfg.n_embd_common
        self._fit_workspace(B, T1, 1, A)
        h_s = torch.empty(B, E, device=self.device, dtype=torch.float32) if raw_tokens is not None else None
        h_e = torch.empty(B, E, device=self.device, dtype=torch.float32) if atoms is not None else None
        if coords is not None:
            coords = coords.to(self.device, torch.float32).contiguous()
        self._keep = (raw_tokens, atoms, coords)
        _lib.check(self.l.coati_engine_encode(self.h, ptr(self.workspace), self.workspace.numel(), B, T1, A, ptr(raw_tokens),
                                              ptr(atoms), ptr(coords), ptr(h_s), ptr(h_e), ptr(self.scal), stream()),
                   "coati_engine_encode")
        self._shape = None
        return h_s, h_e

    def _encode_packed(self, raw_tokens, rows1):
        assert raw_tokens.dtype == torch.int64 and raw_tokens.is_cuda and raw_tokens.is_contiguous() and raw_tokens.dim() == 2
        B, T1 = raw_tokens.shape
        self._fit_workspace(B, T1, 1, 1)
        h_s = torch.empty(B, self.cfg.n_embd_common, device=self.device, dtype=torch.float32)
        self._keep = (raw_tokens,)
        _lib.check(self.l.coati_engine_encode_packed(self.h, ptr(self.workspace), self.workspace.numel(), B, T1, ptr(raw_tokens), rows1,
                                                     ptr(h_s), ptr(self.scal), stream()), "coati_engine_encode_packed")
        self._shape = None
        return h_s

    def decoder_logits(self, tokens, injection=None):
        """RotarySmilesTransformer.forward (injection None) / forward_with_replacement (injection [B, C]: row b's vector at every [UNK]
        position of row b): the decoder pass over the padded tokens [B, T] and the lm_head -> f32 logits [B, T, n_tok] (a view with a
        padded row stride).  COATI1 and COATI2 engines; nothing is kept for a backward."""
        assert tokens.dtype == torch.int64 and tokens.is_cuda and tokens.is_contiguous() and tokens.dim() == 2
        B, T = tokens.shape
        injection = self._injection(injection, B)
        self._fit_workspace(B, 1, T, 1)
        out, ld, logits = self._logits_rows(B * T)
        self._keep = (tokens, injection)
        _lib.check(self.l.coati_engine_decoder_logits(self.h, ptr(self.workspace), self.workspace.numel(), B, T, ptr(tokens), ptr(injection),
                                                      ptr(out), ld, ptr(self.scal), stream()), "coati_engine_decoder_logits")
        self._shape = None
        return logits.view(B, T, self.cfg.n_tok)

    def token_head(self, h):
        """COATI2 coati_to_token (SwiGLUResNet(E, E), simple_coati2/transformer_only.py:19-36) on h [B, E] -> [B, E] f32; scratch from
        the engine workspace.  COATI2 engines only."""
        h = h.to(self.device, torch.float32).contiguous()
        E = self.cfg.n_embd_common
        assert h.dim() == 2 and h.shape[1] == E, h.shape
        B = int(h.shape[0])
        self._fit_workspace(B, 1, 1, 1)
        out = torch.empty(B, E, device=self.device, dtype=torch.float32)
        self._keep = (h,)
        _lib.check(self.l.coati_engine_token_head(self.h, ptr(self.workspace), self.workspace.numel(), B, ptr(h), ptr(out), stream()),
                   "coati_engine_token_head")
        self._shape = None
        return out

    def _score_args(self, tokens, y_next, h, raw_tokens, weights, rows):
        """What the scoring calls share: the checks of the token tensors, the embedding / weights as contiguous f32 device tensors, the
        workspace for (B, T1, T2) and the packed row counts (0, 0 = padded rows).  Returns (B, T1, T2, h, weights, r1, r2)."""
        B, T2 = tokens.shape
        T1 = raw_tokens.shape[1] if raw_tokens is not None else 1
        for t in (tokens, y_next) + ((raw_tokens,) if raw_tokens is not None else ()):
            assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.shape[0] == B
        assert y_next.shape == tokens.shape
        if h is not None:
            h = h.to(self.device, torch.float32).contiguous()
            assert h.shape == (B, self.cfg.n_embd_common)
        if weights is not None:
            weights = weights.to(self.device, torch.float32).contiguous()
            assert weights.shape == (B,)
        self._ensure_workspace(B, T1, T2, 1)
        r1 = r2 = 0
        if rows is not None:
            r1, r2 = (int(x) for x in (rows.tolist() if isinstance(rows, torch.Tensor) else rows))
            if raw_tokens is None:
                r1 = 0
            if r2 <= 0 or (raw_tokens is not None and r1 <= 0):
                r1 = r2 = 0
        return B, T1, T2, h, weights, r1, r2

    def _score(self, entry, tokens, y_next, h, raw_tokens, rows):
        B, T1, T2, h, _, r1, r2 = self._score_args(tokens, y_next, h, raw_tokens, None, rows)
        nll = torch.empty(B, device=self.device, dtype=torch.float32)
        self._keep = (raw_tokens, h, tokens, y_next)
        _lib.check(getattr(self.l, entry)(self.h, ptr(self.workspace), self.workspace.numel(), B, T1, T2, ptr(raw_tokens), ptr(h), ptr(tokens),
                                          ptr(y_next), r1, r2, ptr(nll), ptr(self.scal), stream()), entry)
        self._shape = None
        return nll

    def _score_grad(self, entry, tokens, y_next, h, weights, rows):
        B, _, T2, h, weights, _, r2 = self._score_args(tokens, y_next, h, None, weights, rows)
        nll = torch.empty(B, device=self.device, dtype=torch.float32)
        dh = torch.empty(B, self.cfg.n_embd_common, device=self.device, dtype=torch.float32)
        self._keep = (h, tokens, y_next, weights)
        _lib.check(getattr(self.l, entry)(self.h, ptr(self.workspace), self.workspace.numel(), B, T2, ptr(h), ptr(tokens), ptr(y_next), r2,
                                          ptr(weights), ptr(nll), ptr(dh), ptr(self.scal), stream()), entry)
        self._shape = None
        return nll, dh

    def score(self, tokens, y_next, h_clip=None, raw_tokens=None, rows=None):
        """Per-sequence autoregressive NLL [B] f32 of `tokens` [B, T2] against `y_next` [B, T2] (-1 = ignored), with the special-token
        head's image of an embedding injected at the [UNK] positions (clip_e2e.py:634-742): either the caller's `h_clip` [B, E] or
        encode_tokens(`raw_tokens` [B, T1]).  No point encoder, no logits; the sums are deterministic.  rows = (rows1, rows2) from
        coati_amd.synthetic.packed_rows on host tensors: the transformer passes on packed rows (rows1 only matters with raw_tokens).
        Stays on the device (no sync): error_bits() / losses() report a row without [STOP] or a packed-row mismatch."""
        assert (h_clip is None) != (raw_tokens is None), "score: give exactly one of h_clip / raw_tokens"
        return self._score("coati_engine_score", tokens, y_next, h_clip, raw_tokens, rows)

    def score_grad(self, tokens, y_next, h_clip, weights=None, rows=None):
        """(nll [B], dh_clip [B, E]) f32: the per-sequence NLL of score(tokens, y_next, h_clip=h_clip) -- the same bits -- and
        dh_clip[b] = weights[b] * d nll[b] / d h_clip[b] (weights [B] f32, None = ones), through the decoder pass and the special-token
        head, summed over row b's [UNK] positions (coati_engine_score_grad).  The model is a constant: nothing of params / grads / Adam
        state is written, a train=False engine serves, and backward() afterwards is refused as after score().  rows as in score() (only
        rows2 matters).  Stays on the device (no sync); COATI2 and fp8 engines raise."""
        return self._score_grad("coati_engine_score_grad", tokens, y_next, h_clip, weights, rows)

    def score_coati2(self, tokens, y_next, h_coati=None, raw_tokens=None, rows=None):
        """score() of a COATI2 engine (coati_engine_score_coati2): the embedding is the caller's `h_coati` [B, E] or
        smiles_to_coati of the encoder pass over `raw_tokens` [B, T1], and coati_to_token of it is injected at the [UNK] positions.
        Everything else as in score(); a COATI1 engine raises."""
        assert (h_coati is None) != (raw_tokens is None), "score_coati2: give exactly one of h_coati / raw_tokens"
        return self._score("coati_engine_score_coati2", tokens, y_next, h_coati, raw_tokens, rows)

    def score_grad_coati2(self, tokens, y_next, h_coati, weights=None, rows=None):
        """(nll [B], dh_coati [B, E]) f32 on a COATI2 engine (coati_engine_score_grad_coati2): the NLL of
        score_coati2(tokens, y_next, h_coati=h_coati) -- the same bits -- and dh_coati[b] = weights[b] * d nll[b] / d h_coati[b] through
        the decoder pass and coati_to_token.  Everything else as in score_grad(); a COATI1 engine raises."""
        return self._score_grad("coati_engine_score_grad_coati2", tokens, y_next, h_coati, weights, rows)

    def logits(self):
        if getattr(self, "_packed", False):
            raise RuntimeError("logits(): the last forward ran on packed rows; call forward(..., rows=None)")
        B, _, T2, _ = self._shape
        out, ld, logits = self._logits_rows(B * T2)
        _lib.check(self.l.coati_engine_logits(self.h, ptr(out), ld, stream()), "coati_engine_logits")
        return logits.view(B, T2, self.cfg.n_tok)

    def infonce(self, s_loc, c_loc, s_all, c_all, bad_all, row0=0, gscale=1.0):
        B, Bg = s_loc.shape[0], s_all.shape[0]
        E = self.cfg.n_embd_common
        dS = torch.empty(Bg, E, device=self.device, dtype=torch.float32)
        dC = torch.empty(Bg, E, device=self.device, dtype=torch.float32)
        _lib.check(self.l.coati_engine_infonce(self.h, ptr(s_loc), ptr(c_loc), ptr(s_all), ptr(c_all), ptr(bad_all), B, Bg,
                                               row0, float(gscale), ptr(dS), ptr(dC), ptr(self.scal), stream()),
                   "coati_engine_infonce")
        return dS, dC

    def backward(self, dh_smiles=None, dh_e3gnn=None, stage=0):
        _lib.check(self.l.coati_engine_backward(self.h, ptr(dh_smiles), ptr(dh_e3gnn), stage, stream()), "coati_engine_backward")

    def optimizer_step(self, lr, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1, max_norm=10.0):
        self.step_count += 1
        _lib.check(self.l.coati_engine_optimizer_step(self.h, float(lr), betas[0], betas[1], eps, weight_decay, max_norm,
                                                      self.step_count, ptr(self.scal), stream()), "coati_engine_optimizer_step")

    def error_bits(self):
        """the step's device-side error word as one float per bit [a row without [STOP], packed-row mismatch, atomic number outside the
        nn.Embedding table (torch_emb)] on the device (no sync)"""
        w = self.scal[SCAL_ERR:SCAL_ERR + 1].view(torch.int32)
        return torch.cat([w & 1, (w >> 1) & 1, (w >> 2) & 1]).to(torch.float32)

    def set_error_word(self, bits):
        """bits: the two flags of error_bits() reduced over the ranks; replaces this rank's word before optimizer_step (every rank
        drops the update or none does) and in scal, so that losses() raises on every rank"""
        w = (bits[0:1] > 0).to(torch.int32) + 2 * (bits[1:2] > 0).to(torch.int32) + 4 * (bits[2:3] > 0).to(torch.int32)
        _lib.check(self.l.coati_engine_set_error_word(self.h, ptr(w), stream()), "coati_engine_set_error_word")
        self._err_word_keepalive = w

    def token_entropy_unit(self):
        return math.log(float(self.cfg.n_tok)) / math.log(2.0)

    def train_step(self, batch, use_point, lr, do_clip=True, clip_weight=None, optimizer=True, head="infonce", dh_coati=None, **opt_kw):
        """One single-GPU do_minibatch (train_coati.py:216-277).  Losses stay on the device in self.scal.
        head: "infonce" (clip_e2e.py:27-47) or "barlow" (BASELINE configs[3]; parity unpinned, see barlow.py).
        opt_kw: weight_decay / max_norm / betas / eps forwarded to optimizer_step (train_coati.py:145-151, 276).
        COATI2 engine (train=True): batch = {raw_tokens, tokens, y_next[, rows]}, use_point = None, do_clip=False (True raises
        ValueError); dh_coati [B, E] (optional) is an external gradient w.r.t. h_coati added in the backward.  Returns (zeros, h_coati, bad)."""
        if _coati2_step(self.cfg, do_clip):
            h_e, h_s, bad = self.forward(batch["raw_tokens"], batch["tokens"], y_next=batch["y_next"], train=True, rows=batch.get("rows"))
            if dh_coati is not None:
                dh_coati = dh_coati.to(self.device, torch.float32).contiguous()
                assert dh_coati.shape == h_s.shape, dh_coati.shape
            self.backward(dh_coati, None, 0)
            if optimizer:
                self.optimizer_step(lr, **opt_kw)
            return h_e, h_s, bad
        assert dh_coati is None, "dh_coati belongs to a COATI2 engine"
        h_e, h_s, bad = self.forward(batch["raw_tokens"], batch["tokens"], batch["atoms"], batch["coords"], use_point,
                                     y_next=batch["y_next"], train=True, rows=batch.get("rows"), stop_after_heads=True)
        w = self.token_entropy_unit() if clip_weight is None else clip_weight

        def head_fn():
            if do_clip and head == "barlow":
                from .barlow import barlow_head
                return barlow_head(h_s, h_e, bad, gscale=w)
            if do_clip:
                return (None,) + tuple(self.infonce(h_s, h_e, h_s, h_e, bad, row0=0, gscale=0.5 * w))
            return None, None, None
        # the contrastive head needs the embeddings only: it runs on a side stream underneath the decoder pass
        loss_b, dS, dC = self.contrastive_under_decoder(head_fn)
        if head == "barlow" and do_clip:
            self.barlow_loss = loss_b
        self.backward(dS, dC, 0)
        if optimizer:
            self.optimizer_step(lr, **opt_kw)
        return h_e, h_s, bad

    def eval_step(self, batch, use_point, do_clip=True):
        """Forward + both losses, no backward (the reference's test partition runs under torch.no_grad()).  COATI2 engine
        (train=True): use_point = None, do_clip=False; the AR loss alone."""
        if _coati2_step(self.cfg, do_clip):
            return self.forward(batch["raw_tokens"], batch["tokens"], y_next=batch["y_next"], train=False, rows=batch.get("rows"))
        h_e, h_s, bad = self.forward(batch["raw_tokens"], batch["tokens"], batch["atoms"], batch["coords"], use_point,
                                     y_next=batch["y_next"], train=False, rows=batch.get("rows"))
        if do_clip:
            self.infonce(h_s, h_e, h_s, h_e, bad, row0=0, gscale=0.0)
        return h_e, h_s, bad

    def losses(self):
        """Host copy of the loss scalars of the last step (synchronises)."""
        s = self.scal.detach().cpu()
        err = int(s[SCAL_ERR:SCAL_ERR + 1].view(torch.int32)[0])
        if err & 1:
            raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
        if err & 2:
            raise RuntimeError("packed rows: the row counts passed to forward() differ from what the device found in the tokens")
        if err & 4:
            raise RuntimeError(ERR_Z_MESSAGE)
        ar = float(s[SCAL_AR_SUM] / s[SCAL_AR_COUNT]) if s[SCAL_AR_COUNT] > 0 else 0.0
        nv = float(s[SCAL_NVALID])
        clip = float(0.5 * (s[SCAL_CLIP1] + s[SCAL_CLIP2]) / nv) if nv > 0 else 0.0
        return {"ar_loss": ar, "clip_loss": clip, "loss": ar + clip * self.token_entropy_unit(),
                "grad_norm": float(s[SCAL_GRADNORM]), "n_targets": float(s[SCAL_AR_COUNT]), "n_valid": nv}


    # ---- inference: KV-cached decode ---------------------------------------------------------------
    def decode_begin(self, B, Tmax=None):
        """Start a generation session for B sequences of at most Tmax positions (default n_seq)."""
        Tmax = int(Tmax or self.cfg.n_seq)
        n = int(self.l.coati_engine_decode_workspace_bytes(self.h, int(B), Tmax))
        if n <= 0:
            raise RuntimeError("decode_begin: bad shape")
        self._dec_ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._dec_B = int(B)
        self._dec_Tmax = Tmax
        _lib.check(self.l.coati_engine_decode_begin(self.h, ctypes.c_void_p(self._dec_ws.data_ptr()), n, int(B), Tmax), "decode_begin")

    def decode_step(self, tokens, injection=None, want_logits=True, graph=False):
        """Append one position: tokens [B] int64 (rows equal to the [UNK] id read `injection` [B, C] instead of the
        embedding table).  Returns logits [B, n_tok] f32 or None.  graph=True replays the captured HIP graph
        (decode_graph_build first; must run on a non-default stream); the logits are then a view into the session's
        buffer, valid until the next step."""
        B = self._dec_B
        tokens = tokens.to(self.device, torch.long).contiguous()
        assert tokens.shape == (B,)
        inj = self._injection(injection, B)
        if graph:
            V = self.cfg.n_tok
            lp, ld = ctypes.c_void_p(), ctypes.c_int64()
            _lib.check(self.l.coati_engine_decode_graph_step(self.h, ptr(tokens), ptr(inj), ctypes.byref(lp), ctypes.byref(ld), stream()),
                       "decode_graph_step")
            off = lp.value - self._dec_ws.data_ptr()
            return self._dec_ws[off: off + B * ld.value * 4].view(torch.float32).view(B, ld.value)[:, :V]
        buf, ld, logits = self._logits_rows(B, want_logits)
        _lib.check(self.l.coati_engine_decode_step(self.h, ptr(tokens), ptr(inj), ptr(buf), ld, stream()), "decode_step")
        return logits

    def decode_prefill(self, tokens, injection=None, want_logits=True):
        """Positions 0..m-1 of a fresh session (decode_begin) in ONE transformer pass over tokens [B, m] int64 instead of m
        decode_step calls; rows equal to the [UNK] id read `injection` [B, C] as in decode_step.  Returns the logits
        [B, n_tok] f32 of position m - 1 (or None); the session continues at position m.  Uses the engine's step workspace
        (nothing is kept for a backward); refused on fp8 engines (the step's products are bf16)."""
        B = self._dec_B
        tokens = tokens.to(self.device, torch.long).contiguous()
        assert tokens.dim() == 2 and tokens.shape[0] == B, tokens.shape
        m = int(tokens.shape[1])
        inj = self._injection(injection, B)
        self._ensure_workspace(B, 1, m, 1)
        buf, ld, logits = self._logits_rows(B, want_logits)
        self._keep = (tokens, inj)
        _lib.check(self.l.coati_engine_decode_prefill(self.h, ptr(self.workspace), self.workspace.numel(), ptr(tokens), m, ptr(inj),
                                                      ptr(buf), ld, stream()), "decode_prefill")
        self._shape = None
        return logits

    # ---- ragged sessions: every row at its own position -------------------------------------------------------------
    def decode_step_rows(self, tokens, pos, injection=None, inj_len=None, want_logits=True):
        """decode_step with a position per row: row b appends tokens[b] at pos[b] and attends to 0 .. pos[b].  pos: int32 [B] on the
        device (the caller's; nothing is advanced here); pos[b] < 0 marks an idle slot: its cache is untouched and its logits row
        means nothing.  A slot may be set back to position 0 at any step (what lies behind a row's position is never read).
        inj_len (int32 [B], device; optional): row b reads `injection` only while pos[b] < inj_len[b]."""
        B = self._dec_B
        tokens = tokens.to(self.device, torch.long).contiguous()
        assert tokens.shape == (B,)
        assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.shape == (B,) and pos.device == tokens.device, "pos: int32 [B] on the device"
        inj = self._injection(injection, B)
        if inj_len is not None:
            assert inj is not None and inj_len.dtype == torch.int32 and inj_len.is_contiguous() and inj_len.shape == (B,)
            assert inj_len.device == tokens.device
        buf, ld, logits = self._logits_rows(B, want_logits)
        _lib.check(self.l.coati_engine_decode_step_rows(self.h, ptr(tokens), ptr(pos), ptr(inj), ptr(inj_len), ptr(buf), ld, stream()),
                   "decode_step_rows")
        return logits

    def decode_prefill_rows(self, prompt, plen, injection=None, want_logits=True):
        """Every row's WHOLE prompt of a fresh session in one transformer pass on packed rows: prompt [B, W] int64 (row b counts
        plen[b] tokens, whatever their ids), plen [B] with 1 <= plen[b] <= W <= Tmax.  Returns the logits [B, n_tok] f32 of position
        plen[b] - 1 (or None); continue with decode_step_rows at pos[b] = plen[b].  Refused behind any step and on fp8 engines."""
        B = self._dec_B
        prompt = prompt.to(self.device, torch.long).contiguous()
        assert prompt.dim() == 2 and prompt.shape[0] == B, prompt.shape
        W = int(prompt.shape[1])
        plen_h = plen.detach().to("cpu", torch.int64)
        assert plen_h.shape == (B,)
        Tmax = self._dec_Tmax
        if int(plen_h.min()) < 1 or int(plen_h.max()) > min(W, Tmax):
            raise ValueError(f"decode_prefill_rows: prompt lengths {int(plen_h.min())} .. {int(plen_h.max())}; 1 .. {min(W, Tmax)} fit")
        plen_d = plen.to(self.device, torch.int32).contiguous()
        inj = self._injection(injection, B)
        self._ensure_workspace(B, 1, W, 1)
        buf, ld, logits = self._logits_rows(B, want_logits)
        self._keep = (prompt, plen_d, inj)
        _lib.check(self.l.coati_engine_decode_prefill_rows(self.h, ptr(self.workspace), self.workspace.numel(), ptr(prompt), W, ptr(plen_d),
                                                           int(plen_h.sum()), ptr(inj), ptr(buf), ld, stream()), "decode_prefill_rows")
        self._shape = None
        return logits

    def _sample_rows(self, logits, k, inv_temp, u, ldu, prompt, plen, req, pos, out, tok_next, done, Tmax, stop_token):
        """coati_topk_sample_rows on the session's B slots (see include/coati_hip.h)."""
        _lib.call("coati_topk_sample_rows", ptr(logits), logits.stride(0), int(logits.shape[0]), self.cfg.n_tok, int(k), float(inv_temp),
                  ptr(u), int(ldu), ptr(prompt), int(prompt.stride(0)) if prompt is not None else 0, ptr(plen), ptr(req), ptr(pos), ptr(out),
                  int(out.stride(0)), ptr(tok_next), ptr(done), int(Tmax), int(stop_token), stream())

    def decode_graph_build(self):
        """Capture the decode step into HIP graphs (call inside `with torch.cuda.stream(side_stream)`)."""
        _lib.check(self.l.coati_engine_decode_graph_build(self.h, stream()), "decode_graph_build")

    def generate_top_k_with_inj_batch(self, prefix, stop_token, pad_token=0, inv_temp=1.0, k=50, inj_token=None,
                                      inj_payload=None, as_tensor=False, generator=None, use_graph=False, grammar=None):
        """See _generate; runs on a private stream so that the decode step can be replayed from a captured HIP graph
        (use_graph=True).  Measured: replay == eager (the step is bound by the ~6 us device-side cost of each of its ~115
        dependent kernels, not by host launch overhead), so eager is the default.
        grammar (a coati_amd.grammar.SmilesGrammar): only tokens that keep parentheses, ring digits and bracket atoms closable
        within n_seq are drawn, so every row draws its own [STOP]; rows whose prefix already broke the syntax are unconstrained and
        marked in last_grammar_violations (bool [B]).  Not with use_graph."""
        if grammar is not None and use_graph:
            raise NotImplementedError("grammar= with use_graph=True: the mask launch is not part of the captured decode graphs")
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            out = self._generate(prefix, stop_token, pad_token, inv_temp, k, inj_token, inj_payload, as_tensor, generator, use_graph,
                                 grammar)
        torch.cuda.current_stream(self.device).wait_stream(side)
        return out

    def _grammar_begin(self, grammar, stop_token, rows, remaining):
        """The device states [B, 4] behind the forced token lists `rows` (one list: every row of the batch alike), `remaining` positions
        to fill from their first token on."""
        if int(stop_token) != grammar.stop_token or grammar.n_token != self.cfg.n_tok:
            raise ValueError(f"grammar: built for {grammar.n_token} tokens with [STOP] = {grammar.stop_token}; the call has "
                             f"{self.cfg.n_tok} and {int(stop_token)}")
        return grammar.states([grammar.walk(r, remaining) for r in rows], self.device)

    def _grammar_end(self, grammar, logits, state, tok_last):
        """Advances the states by the last tokens (what is still open behind the last position is a violation) and returns the dead
        rows, bool [B].  The consumed logits serve as the launch's operand."""
        grammar.step(logits, state, state, tok_prev=tok_last, remaining=1)
        return (state[:, 2] & 2) != 0

    def _generate(self, prefix, stop_token, pad_token, inv_temp, k, inj_token, inj_payload, as_tensor, generator, use_graph,
                  grammar=None):
        """RotarySmilesTransformer.generate_top_k_with_inj_batch (smiles_xformer.py:272-351) on the KV-cached decode
        path: same arguments, same stopping rules (stopped rows emit pad_token, rows that never stop get a final
        stop_token), sampling = softmax(top-k logits * inv_temp) drawn with uniforms from `generator`."""
        prefix = [int(t) for t in prefix]
        B = int(inj_payload.shape[0])
        if inj_token is not None and int(inj_token) != self.cfg.unk_token:
            raise NotImplementedError("the injection slot must be the engine's [UNK] id")
        n_seq = self.cfg.n_seq
        self.decode_begin(B, n_seq)
        if use_graph:
            self.decode_graph_build()
        dev = self.device
        logits = None
        for i, t in enumerate(prefix):
            tok = torch.full((B,), t, dtype=torch.long, device=dev)
            logits = self.decode_step(tok, inj_payload if (inj_token is not None and t == int(inj_token)) else None,
                                      want_logits=(i == len(prefix) - 1), graph=use_graph)
        stopped = torch.zeros(B, dtype=torch.int32, device=dev)
        generated = []
        idx = 0
        gstate = self._grammar_begin(grammar, stop_token, [prefix], n_seq).repeat(B, 1) if grammar is not None else None
        while idx < n_seq - len(prefix):
            if grammar is not None:   # the state follows the token drawn last; n_seq - len(prefix) - idx positions are still to be drawn
                grammar.step(logits, gstate, gstate, tok_prev=generated[-1] if generated else None, remaining=n_seq - len(prefix) - idx)
            u = torch.rand(B, device=dev, generator=generator) if k > 1 else torch.zeros(B, device=dev)
            nxt = torch.empty(B, dtype=torch.long, device=dev)
            _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, self.cfg.n_tok, int(k), float(inv_temp), ptr(u),
                      ptr(nxt), ptr(stopped), int(stop_token), int(pad_token), stream())
            generated.append(nxt)
            idx += 1
            if int(stopped.sum().item()) >= B or idx >= n_seq - len(prefix):
                break
            logits = self.decode_step(nxt, graph=use_graph)
        gen = torch.stack(generated, dim=1)
        not_stopped = stopped == 0
        self.last_unstopped = not_stopped            # bool [B]: the rows whose last position is overwritten with [STOP] below
        self.last_grammar_violations = self._grammar_end(grammar, logits, gstate, generated[-1]) if grammar is not None else None
        if bool(not_stopped.any()):
            gen[not_stopped, -1] = int(stop_token)
        if as_tensor:
            return torch.cat([torch.tensor(prefix, dtype=torch.long, device=dev).unsqueeze(0).repeat(B, 1), gen], dim=1)
        return [prefix + row for row in gen.tolist()]

    # ---- beam search (include/coati_beam.h) ----------------------------------------------------------------------------
    def decode_step_beams(self, tokens, anc, injection=None, want_logits=True):
        """decode_step with every layer's attention in ancestry mode (coati_engine_decode_step_beams): position t of row b is read
        from cache row anc[b, t] (int32 [B, Tmax] on the device), the new record is appended in row b.  Advances the session."""
        B = self._dec_B
        tokens = tokens.to(self.device, torch.long).contiguous()
        assert tokens.shape == (B,)
        assert anc.dtype == torch.int32 and anc.is_contiguous() and anc.shape == (B, self._dec_Tmax) and anc.device == tokens.device, \
            "anc: int32 [B, Tmax] on the device"
        inj = self._injection(injection, B)
        buf, ld, logits = self._logits_rows(B, want_logits)
        _lib.call("coati_engine_decode_step_beams", self.h, ptr(tokens), ptr(anc), ptr(inj), ptr(buf), ld, stream())
        return logits

    def beam_search(self, prefix, stop_token, pad_token=0, beams=4, inj_token=None, inj_payload=None, max_len=None, length_penalty=0.0,
                    grammar=None):
        """The `beams` most likely continuations of `prefix` for every row of inj_payload [G, C], by beam search on the KV-cached decode
        path (runs on a private stream, like generate_top_k_with_inj_batch).  Returns (tokens [G, W, T] int64: prefix + generated,
        pad_token behind [STOP]; scores [G, W] f32: the sum of the generated tokens' log-probabilities, [STOP] included; lengths [G, W]:
        generated tokens up to and with [STOP]; finished [G, W] bool), per group sorted by score / max(length, 1) ** length_penalty,
        best first.  The search itself ranks by the raw sum (ties: parent beam, then token id, ascending); the penalty only reorders
        the result.  It ends when every hypothesis has drawn [STOP] or at min(max_len, n_seq) positions; a hypothesis that has not
        finished by then is returned as it stands (finished = False, no [STOP] appended: its score is that of its tokens).
        grammar (a coati_amd.grammar.SmilesGrammar): only continuations that stay closable within the positions left are ranked, and
        a beam's score is the sum of log-probabilities RENORMALISED OVER THE ADMITTED TOKENS of each step (the log-softmax of the
        masked logits), not the model's own; every hypothesis of finite score then ends in [STOP] with everything closed.  Fewer than
        `beams` admitted continuations leave hypotheses of score -inf.  last_grammar_violations: bool [G, W] in the result's order."""
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            out = self._beam_search(prefix, stop_token, pad_token, beams, inj_token, inj_payload, max_len, length_penalty, grammar=grammar)
        torch.cuda.current_stream(self.device).wait_stream(side)
        return out

    def _beam_search(self, prefix, stop_token, pad_token, beams, inj_token, inj_payload, max_len, length_penalty, trace=None,
                     grammar=None):
        """beam_search on the current stream.  trace (a list, for the tests): receives per step (parent rows [B] int32, tokens [B] int64,
        scores [B] f32) of the new rows g * W + rank, on the device."""
        prefix = [int(t) for t in prefix]
        W, V, dev = int(beams), self.cfg.n_tok, self.device
        if not 1 <= W <= 16 or W > V:
            raise ValueError(f"beam_search: beams = {W}; 1 .. min(16, n_tok) fit")
        if inj_token is not None and int(inj_token) != self.cfg.unk_token:
            raise NotImplementedError("the injection slot must be the engine's [UNK] id")
        n_seq = min(int(max_len), self.cfg.n_seq) if max_len else self.cfg.n_seq
        m = len(prefix)
        if not 1 <= m < n_seq:
            raise ValueError(f"beam_search: a prefix of {m} tokens; 1 .. {n_seq - 1} fit")
        G = int(inj_payload.shape[0])
        B = G * W
        payload = self._injection(inj_payload, G).repeat_interleave(W, dim=0)     # row g * W + r reads inj_payload[g]
        Tmax = self.cfg.n_seq
        self.decode_begin(B, Tmax)
        logits = None
        for i, t in enumerate(prefix):
            tok = torch.full((B,), t, dtype=torch.long, device=dev)
            logits = self.decode_step(tok, payload if (inj_token is not None and t == int(inj_token)) else None, want_logits=(i == m - 1))
        steps = n_seq - m
        # state, ping-pong: [cum, fin, len, anc, hist]
        cum = torch.full((G, W), float("-inf"), device=dev)
        cum[:, 0] = 0.0
        ident = torch.arange(B, dtype=torch.int32, device=dev).unsqueeze(1).repeat(1, Tmax).contiguous()
        cur = [cum.view(B), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), ident,
               torch.full((B, steps), int(pad_token), dtype=torch.long, device=dev)]
        nxt = [torch.empty_like(cur[0]), torch.empty_like(cur[1]), torch.empty_like(cur[2]), ident.clone(), cur[4].clone()]
        cand_s = torch.empty(B, W, device=dev)
        cand_t = torch.empty(B, W, dtype=torch.int32, device=dev)
        tok_next = torch.empty(B, dtype=torch.long, device=dev)
        nfin = torch.zeros(G, dtype=torch.int32, device=dev)
        n = 0
        if grammar is not None:   # the automaton states ping-pong through the merge's parent rows, next to anc
            gcur = self._grammar_begin(grammar, stop_token, [prefix], n_seq).repeat(B, 1)
            gnxt = torch.empty_like(gcur)
            parent = None
        while True:
            if grammar is not None:
                grammar.step(logits, gcur, gnxt, tok_prev=tok_next if n else None, parent=parent, remaining=steps - n)
                gcur, gnxt = gnxt, gcur
            _lib.call("coati_beam_row_topk", ptr(logits), logits.stride(0), G, W, V, ptr(cur[0]), ptr(cur[1]), int(pad_token), ptr(cand_s),
                      ptr(cand_t), stream())
            _lib.call("coati_beam_merge", ptr(cand_s), ptr(cand_t), G, W, ptr(cur[0]), ptr(cur[1]), ptr(cur[2]), ptr(cur[3]), ptr(cur[4]),
                      steps, Tmax, m - 1 + n, n, int(stop_token), ptr(nxt[0]), ptr(nxt[1]), ptr(nxt[2]), ptr(nxt[3]), ptr(nxt[4]),
                      ptr(tok_next), ptr(nfin), stream())
            cur, nxt = nxt, cur
            if grammar is not None:
                parent = cur[3][:, m - 1 + n].contiguous()
            if trace is not None:
                trace.append((cur[3][:, m - 1 + n].clone(), tok_next.clone(), cur[0].clone()))
            n += 1
            if n >= steps or int(nfin.sum().item()) >= B:
                break
            logits = self.decode_step_beams(tok_next, cur[3])
        scores, fin, lens, hist = cur[0].view(G, W), cur[1].view(G, W) != 0, cur[2].view(G, W), cur[4][:, :n].reshape(G, W, n)
        key = scores / lens.clamp(min=1).to(torch.float32) ** float(length_penalty)
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        self.last_grammar_violations = None
        if grammar is not None:
            grammar.step(logits, gcur, gnxt, tok_prev=tok_next, parent=parent, remaining=1)
            self.last_grammar_violations = torch.gather(((gnxt[:, 2] & 2) != 0).view(G, W), 1, order)
        head = torch.tensor(prefix, dtype=torch.long, device=dev).view(1, 1, m).expand(G, W, m)
        tokens = torch.cat([head, torch.gather(hist, 1, order.unsqueeze(2).expand(G, W, n))], dim=2)
        return tokens, torch.gather(scores, 1, order), torch.gather(lens, 1, order), torch.gather(fin, 1, order)

    def generate_topk_batch(self, prefix, stop_token, pad_token=0, inv_temp=2, k=10, generator=None, prefill=True, ragged=False,
                            grammar=None):
        """RotarySmilesTransformer.generate_topk_batch (smiles_xformer.py:157-198): continue B prompts of different lengths
        (token lists) on the KV-cached decode path.  Returns B lists of n_seq ints: every prompt verbatim, each row sampled
        from its own prompt end (softmax(top-k logits * inv_temp), uniforms from `generator`), [STOP] and then pad_token,
        zeros behind the last written column.  The loop ends when every row has stopped or column n_seq - 1 is written.
        prefill=True runs the shortest prompt's length as one pass (decode_prefill); the longer prompts' remaining tokens,
        and with prefill=False every prompt token behind the first, are fed through forced steps.
        ragged=True: every prompt is prefilled in FULL (decode_prefill_rows) and the rows then step at their own positions, each
        sampling from its own prompt end at once; a row is done when it draws [STOP], and the call when every row is.  Same output
        format.  Off by default: with k > 1 the uniforms reach the rows in another order, so a seed's samples differ from the
        aligned path's.  (fp8 engines: the prompts go through forced ragged steps.)
        grammar (a coati_amd.grammar.SmilesGrammar; aligned path only): the prompt's tokens advance each row's automaton state, and only
        tokens that keep the row closable within n_seq are drawn -- the completion of `c1ccc(` closes it.  A prompt that breaks the
        syntax itself (`)`) leaves its row unconstrained and marked in last_grammar_violations (bool [B])."""
        out, _ = self._complete(prefix, stop_token, pad_token, inv_temp, k, generator, prefill, None, ragged, grammar)
        return out.tolist()

    def generate_topk_with_inj(self, prefix, stop_token, inv_temp=1, k=50, inj_token=None, inj_payload=None, generator=None,
                               prefill=True, grammar=None):
        """RotarySmilesTransformer.generate_topk_with_inj (smiles_xformer.py:215-270): one prompt (token list) whose
        inj_token slot carries inj_payload ([C], or a scalar that fills all C channels, as the reference's assignment
        broadcasts it); sampling stops on stop_token or after n_seq - 1 generated tokens.  Returns prefix + generated.
        A sequence that has not stopped within n_seq positions is returned at n_seq positions (the reference raises).
        grammar: as in generate_topk_batch."""
        prefix = [int(t) for t in prefix]
        C = self.cfg.n_hidden_xformer
        inj = None
        if inj_token is not None:
            if int(inj_token) != self.cfg.unk_token:
                raise NotImplementedError("the injection slot must be the engine's [UNK] id")
            if int(inj_token) not in prefix:
                raise ValueError(f"{inj_token} is not in the prefix")
            p = torch.as_tensor(inj_payload).to(self.device, torch.float32).reshape(-1)
            if p.numel() == 1:
                p = p.expand(C)
            assert p.numel() == C, f"inj_payload: {p.numel()} values for {C} channels"
            inj = p.reshape(1, C).contiguous()
        out, n = self._complete([prefix], stop_token, 0, inv_temp, k, generator, prefill, inj, grammar=grammar)
        return out[0, :n].tolist()

    def _complete(self, prefix, stop_token, pad_token, inv_temp, k, generator, prefill, injection, ragged=False, grammar=None):
        """The decode loop of generate_topk_batch / generate_topk_with_inj on a private stream.  Returns (tokens [B, n_seq] on
        the host, number of columns written)."""
        if grammar is not None and ragged:
            raise NotImplementedError("grammar= with ragged=True: the ragged sampler draws and advances in one launch")
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            if ragged:
                out = self._complete_rows_on_stream(prefix, stop_token, pad_token, inv_temp, k, generator, prefill, injection)
            else:
                out = self._complete_on_stream(prefix, stop_token, pad_token, inv_temp, k, generator, prefill, injection, grammar)
        torch.cuda.current_stream(self.device).wait_stream(side)
        return out

    def _complete_on_stream(self, prefix, stop_token, pad_token, inv_temp, k, generator, prefill, injection, grammar=None):
        n_seq = int(self.cfg.n_seq)
        prompt, plen = pack_prompts(prefix, n_seq)
        B = prompt.shape[0]
        m, longest = int(plen.min()), int(plen.max())
        dev = self.device
        prompt_d, plen_d = prompt.to(dev), plen.to(dev)
        out = torch.zeros(B, n_seq, dtype=torch.long, device=dev)
        out[:, :m] = prompt_d[:, :m]
        stopped = (prompt[:, :m] == int(stop_token)).any(1).to(torch.int32).to(dev)
        self.decode_begin(B, n_seq)
        if prefill and not self.cfg.fp8:
            logits = self.decode_prefill(prompt_d[:, :m], injection)
            pos = m
        else:   # (fp8 engines: the prompt goes through forced steps)
            logits = self.decode_step(out[:, 0], injection)
            pos = 1
        nxt = None
        self.last_grammar_violations = None
        if grammar is not None:   # the state behind the columns fed so far; forced prompt tokens behind them advance it like drawn ones
            gstate = self._grammar_begin(grammar, stop_token, [r[:pos] for r in prompt.tolist()], n_seq)
        while pos < n_seq:
            if grammar is not None:
                grammar.step(logits, gstate, gstate, tok_prev=nxt, remaining=n_seq - pos)
            u = torch.rand(B, device=dev, generator=generator) if k > 1 else torch.zeros(B, device=dev)
            nxt = torch.empty(B, dtype=torch.long, device=dev)
            _lib.call("coati_topk_sample_prompt", ptr(logits), logits.stride(0), B, self.cfg.n_tok, int(k), float(inv_temp), ptr(u),
                      ptr(prompt_d), n_seq, ptr(plen_d), pos, ptr(nxt), ptr(stopped), int(stop_token), int(pad_token), stream())
            out[:, pos] = nxt
            pos += 1
            if pos >= n_seq or (pos >= longest and int(stopped.sum().item()) >= B):
                break
            logits = self.decode_step(nxt, injection)
        if grammar is not None:
            self.last_grammar_violations = self._grammar_end(grammar, logits, gstate, nxt)
        return out.cpu(), pos

    def _complete_rows_on_stream(self, prefix, stop_token, pad_token, inv_temp, k, generator, prefill, injection):
        """_complete_on_stream on a ragged session: the whole of every prompt in one packed pass, then steps in which row b sits at
        its own position.  Returns (tokens [B, n_seq] on the host, number of columns written)."""
        n_seq = int(self.cfg.n_seq)
        prompt, plen = pack_prompts(prefix, n_seq)
        B = prompt.shape[0]
        longest = int(plen.max())
        dev = self.device
        prompt_d, plen_d = prompt.to(dev), plen.to(dev)
        out = prompt_d.clone()                       # prompts verbatim (zeros behind them)
        cols = torch.arange(n_seq).unsqueeze(0)
        in_prompt = (prompt == int(stop_token)) & (cols < plen.unsqueeze(1))
        has_stop = in_prompt.any(1)
        first_stop = torch.where(has_stop, in_prompt.to(torch.int64).argmax(1) + 1, torch.zeros(B, dtype=torch.int64))
        self.decode_begin(B, n_seq)
        tok = prompt_d[:, 0].clone()
        done = torch.zeros(B, dtype=torch.int32, device=dev)
        if prefill and not self.cfg.fp8:
            logits = self.decode_prefill_rows(prompt_d[:, :longest], plen_d, injection)
            # a prompt that holds a [STOP] is a finished row (its slot stays idle); a prompt of n_seq tokens is retired by the sampler
            pos_h = torch.where(has_stop, torch.full((B,), -1, dtype=torch.int64), plen.to(torch.int64) - 1)
            done_h = torch.where(has_stop, first_stop, torch.zeros(B, dtype=torch.int64))
        else:   # (fp8 engines: the prompt goes through forced ragged steps; the sampler's prompt rule ends a row at a [STOP] in it)
            stop0 = prompt[:, 0] == int(stop_token)
            pos_h = torch.where(stop0, torch.full((B,), -1, dtype=torch.int64), torch.zeros(B, dtype=torch.int64))
            done_h = stop0.to(torch.int64)
            logits = None
        pos = pos_h.to(torch.int32).to(dev)
        done.copy_(done_h.to(torch.int32))
        if logits is None:
            logits = self.decode_step_rows(tok, pos, injection)
        while True:
            u = torch.rand(B, device=dev, generator=generator) if k > 1 else torch.zeros(B, device=dev)
            self._sample_rows(logits, k, inv_temp, u, 0, prompt_d, plen_d, None, pos, out, tok, done, n_seq, stop_token)
            if int((pos >= 0).sum().item()) == 0:
                break
            logits = self.decode_step_rows(tok, pos, injection)
        # [STOP], then pad_token up to the column where the longest row ended, zeros behind
        end = torch.maximum(done.to(torch.int64).cpu(), plen.to(torch.int64))
        width = max(longest, int(end.max()))
        out = out.cpu()
        behind = (cols >= end.unsqueeze(1)) & (cols < width)
        out[behind] = int(pad_token)
        return out, width

    def generate_stream(self, prefix, stop_token, pad_token=0, inv_temp=1.0, k=50, inj_token=None, inj_payload=None, slots=None,
                        generator=None, as_tensor=False, poll=1, forced=None, grammar=None):
        """generate_top_k_with_inj_batch for N = inj_payload.shape[0] requests on `slots` cache slots (default min(N,
        slots.STREAM_SLOT_CAP)): a slot whose row has drawn [STOP] is handed the next request at position 0 while the other rows
        carry on, so no step is spent on finished rows as long as requests wait.  A request enters with the first prefix token and
        its own injection row; the rest of the prefix goes through forced steps.  Returns the N rows in REQUEST order, shaped like
        generate_top_k_with_inj_batch's (prefix + generated, pad_token behind [STOP], rows that never stop end in stop_token, width =
        the longest row of the call).  Request n's uniforms are row n of one [N, n_seq] draw from `generator` at the call: they
        depend on n and the position, not on the slot or the step the request ran in.
        poll: the host looks for ended rows every `poll` steps (1: every step, as the aligned loops synchronise every step).
        forced (tokens [N, W], lengths [N]): request n emits tokens[n, :lengths[n]] through the sampler's prompt rule instead of
        the prefix (benchmarks with random weights, which never draw [STOP], force their row lengths with it).
        self.stream_steps holds the number of decode steps the call took.  grammar= is not supported here."""
        if grammar is not None:
            raise NotImplementedError("grammar= with generate_stream / slots=: the ragged sampler draws and advances in one launch")
        from .slots import STREAM_SLOT_CAP, SlotScheduler
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            prefix = [int(t) for t in prefix]
            if inj_token is not None and int(inj_token) != self.cfg.unk_token:
                raise NotImplementedError("the injection slot must be the engine's [UNK] id")
            dev, n_seq, C = self.device, int(self.cfg.n_seq), self.cfg.n_hidden_xformer
            payload = inj_payload.to(dev, torch.float32).contiguous()
            N = int(payload.shape[0])
            assert payload.shape == (N, C) and N > 0
            S = int(slots) if slots is not None else min(N, STREAM_SLOT_CAP)
            if S < 1:
                raise ValueError("generate_stream: at least one slot")
            S = min(S, N)
            if forced is None:
                if not 1 <= len(prefix) <= n_seq:
                    raise ValueError(f"generate_stream: a prefix of {len(prefix)} tokens; 1 .. n_seq = {n_seq} fit")
                prompt_d = torch.tensor(prefix, dtype=torch.long, device=dev).unsqueeze(0).repeat(N, 1)
                plen_d = torch.full((N,), len(prefix), dtype=torch.int32, device=dev)
            else:
                prompt_d = forced[0].to(dev, torch.long).contiguous()
                plen_d = forced[1].to(dev, torch.int32).contiguous()
                assert prompt_d.shape[0] == N and plen_d.shape == (N,) and prompt_d.shape[1] <= n_seq
                assert int(plen_d.min()) >= 1 and int(plen_d.max()) <= prompt_d.shape[1]
            P = int(prompt_d.shape[1])
            u = torch.rand(N, n_seq, device=dev, generator=generator) if k > 1 else None
            out = torch.zeros(N, n_seq, dtype=torch.long, device=dev)
            out[:, 0] = prompt_d[:, 0]
            tok = torch.zeros(S, dtype=torch.long, device=dev)
            pos = torch.full((S,), -1, dtype=torch.int32, device=dev)
            req = torch.zeros(S, dtype=torch.int32, device=dev)
            done = torch.zeros(S, dtype=torch.int32, device=dev)
            inj = torch.zeros(S, C, dtype=torch.float32, device=dev)
            inj_len = torch.zeros(S, dtype=torch.int32, device=dev)
            use_inj = inj_token is not None
            self.decode_begin(S, n_seq)
            sched = SlotScheduler(N, S)
            self.stream_steps = 0

            def step(new):
                if new:
                    sl = torch.tensor([s for s, _ in new], dtype=torch.long, device=dev)
                    rq = torch.tensor([r for _, r in new], dtype=torch.long, device=dev)
                    tok[sl] = prompt_d[rq, 0]
                    pos[sl] = 0
                    req[sl] = rq.to(torch.int32)
                    done[sl] = 0
                    inj[sl] = payload[rq]
                    inj_len[sl] = plen_d[rq]
                logits = self.decode_step_rows(tok, pos, inj if use_inj else None, inj_len if use_inj else None)
                self._sample_rows(logits, k, inv_temp, u, n_seq if u is not None else 0, prompt_d, plen_d, req, pos, out, tok, done, n_seq,
                                  stop_token)
                self.stream_steps += 1
                return []

            lens = [0] * N
            while not sched.finished:
                new = sched.refill()
                for i in range(max(1, int(poll))):
                    step(new if i == 0 else [])
                d = done.cpu()           # (synchronises: the one look per `poll` steps)
                for s in torch.nonzero(d).flatten().tolist():
                    if sched.slot_req[s] >= 0:
                        lens[sched.retire(s)] = int(d[s])
                done.zero_()
            lens_t = torch.tensor(lens, dtype=torch.long, device=dev)
            width = int(lens_t.max())
            gen = out[:, :width].clone()
            if width == n_seq:       # rows that never stopped end in stop_token
                gen[lens_t == n_seq, n_seq - 1] = int(stop_token)
            gen[torch.arange(width, device=dev).unsqueeze(0) >= lens_t.unsqueeze(1)] = int(pad_token)
            res = gen if as_tensor else gen.tolist()
        torch.cuda.current_stream(self.device).wait_stream(side)
        return res

    # ---- profiling ---------------------------------------------------------------------------------------------
    def site_names(self):
        return [self.l.coati_engine_site_name(i).decode() for i in range(self.l.coati_engine_site_count())]

    def prof_select(self, site, keep_overlap=False):
        """HIP events around every launch of `site` (-1: off).  keep_overlap: the step keeps running as the product runs it
        (point encoder concurrent on the side stream) -- bench.py's timed region; default: the point encoder is serialised
        so that a site's events bracket its kernels alone (the per-site table)."""
        names = self.site_names()
        sites = [s.strip() for s in site.split(",")] if isinstance(site, str) else [site]     # "fc1_dgrad,qkv_dgrad": several sites at once
        idx = [names.index(s) if isinstance(s, str) else s for s in sites]
        _lib.check(self.l.coati_engine_prof_select(self.h, idx[0]), "prof_select")
        for i in idx[1:]:
            _lib.check(self.l.coati_engine_prof_add_site(self.h, i), "prof_add_site")
        if keep_overlap:
            _lib.check(self.l.coati_engine_prof_keep_overlap(self.h, 1), "prof_keep_overlap")

    def prof_pause(self, paused=True):
        """suspend / resume the selected sites' events (selection and counters stay): sampling a subset of the steps"""
        _lib.check(self.l.coati_engine_prof_pause(self.h, 1 if paused else 0), "prof_pause")

    def prof_collect(self):
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(self.l.coati_engine_prof_collect(self.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "prof_collect")
        return ms.value, n.value, fl.value

    def prof_last_bytes(self):
        """Algorithmic HBM bytes per launch of the site returned by the last prof_collect()."""
        b = ctypes.c_double()
        _lib.check(self.l.coati_engine_prof_last_bytes(self.h, ctypes.byref(b)), "prof_last_bytes")
        return b.value
