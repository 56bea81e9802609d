"""Beam search, host side (no GPU): include/coati_beam.h parses against coati_hip.h and the library exports what it declares, the
float64 restatement the GPU tests compare against (tests/beam_util.py) is exact where beam search must be, and the operators refuse bad
arguments with a code before anything is enqueued."""
import ctypes
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import beam_util  # noqa: E402

ENTRIES = ("coati_attn_decode_anc", "coati_beam_row_topk", "coati_beam_merge", "coati_engine_decode_step_beams")


def _headers():
    from coati_amd import _abi, build
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.BEAM_HEADER) as f:
        text = f.read()
    return _abi, base, text


def test_beam_header_parses_against_the_first_header():
    _abi, base, text = _headers()
    beam = _abi.parse(text, guard="COATI_BEAM_H", name="coati_beam.h", base=base)
    assert sorted(beam.prototypes) == sorted(ENTRIES)
    assert not set(beam.prototypes) & set(base.prototypes)
    assert beam.version == base.version == 5 and beam.CoatiConfig is base.CoatiConfig and not beam.experimental
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert beam.prototypes["coati_attn_decode_anc"] == (I, [P, P, P, I, I, I, I, I, P, P])
    assert beam.prototypes["coati_beam_row_topk"] == (I, [P, L, I, I, I, P, P, I, P, P, P])
    assert beam.prototypes["coati_beam_merge"] == (I, [P, P, I, I, P, P, P, P, P, L, I, I, I, I, P, P, P, P, P, P, P, P])
    assert beam.prototypes["coati_engine_decode_step_beams"] == (I, [P, P, P, P, P, L, P])


def test_reader_names_the_second_header_in_its_errors_and_refuses_a_redeclaration():
    _abi, base, text = _headers()
    marker = "#endif /* COATI_BEAM_H */"
    kw = dict(guard="COATI_BEAM_H", name="coati_beam.h", base=base)
    with pytest.raises(ValueError, match=r"coati_beam\.h: type 'double ' is not one"):
        _abi.parse(text.replace(marker, "int coati_x(double v);\n" + marker), **kw)
    with pytest.raises(ValueError, match=r"coati_beam\.h: coati_gemm_nt is already declared in coati_hip\.h"):
        _abi.parse(text.replace(marker, "int coati_gemm_nt(int a);\n" + marker), **kw)
    with pytest.raises(ValueError, match=r"coati_beam\.h: preprocessor line"):
        _abi.parse(text, name="coati_beam.h", base=base)      # read under the first header's guard: its own #ifndef is unknown
    with pytest.raises(ValueError, match=r"coati_beam\.h: coati_config or a numeric COATI_ABI_VERSION is missing"):
        _abi.parse(text, guard="COATI_BEAM_H", name="coati_beam.h")      # stand-alone: the header defines neither


def test_library_exports_the_beam_entries_and_the_first_table_is_unchanged():
    from coati_amd import _lib
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5
    assert sorted(_lib.BEAM_PROTOTYPES) == sorted(ENTRIES)
    assert not set(_lib.BEAM_PROTOTYPES) & set(_lib.PROTOTYPES) and not set(ENTRIES) & set(_lib.exported_symbols())
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.BEAM_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_operators_refuse_bad_arguments_with_a_code():
    """W = 0, W = 17, W > V, a null ancestry table: a code and a message, decided on the host (the pointers are host buffers that a
    refusal never looks at).  (A ragged session needs a device to come about: tests/test_gpu_beam.py.)"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    buf2 = (ctypes.c_float * 4096)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)

    def topk(W, V):
        return l.coati_beam_row_topk(p, 64, 1, W, V, p, p, 0, p, p, None)

    def merge(W, anc_out=q):
        return l.coati_beam_merge(p, p, 1, W, p, p, p, p, p, 8, 24, 3, 0, 1, q, q, q, anc_out, q, q, q, None)

    for W, V in ((0, 48), (17, 48), (5, 4)):
        assert topk(W, V) == -2 and b"beam_row_topk" in l.coati_last_error(), (W, V)
    for W in (0, 17):
        assert merge(W) == -2 and b"beam_merge" in l.coati_last_error(), W
    assert merge(4, anc_out=None) == -1 and b"null" in l.coati_last_error()
    assert l.coati_attn_decode_anc(p, p, p, 2, 4, 16, 24, 3, None, None) == -1 and b"null ancestry" in l.coati_last_error()
    assert l.coati_attn_decode_anc(p, p, p, 2, 4, 24, 24, 3, p, None) == -2 and b"attn_decode_anc" in l.coati_last_error()
    assert l.coati_engine_decode_step_beams(None, p, p, None, None, 0, None) == -1 and b"decode_step_beams" in l.coati_last_error()
    cfg = _lib.CoatiConfig(2, 2, 128, 64, 128, 8, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 1, 1)
    h = ctypes.c_void_p()
    assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, l.coati_last_error()
    assert l.coati_engine_decode_step_beams(h, p, p, None, None, 0, None) == -1 and b"no decode session" in l.coati_last_error()
    l.coati_engine_destroy(h)
    with pytest.raises(RuntimeError, match="coati_beam_row_topk failed"):
        _lib.call("coati_beam_row_topk", p, 64, 1, 0, 48, p, p, 0, p, p, None)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
V5, STOP5, STEPS5 = 5, 1, 4


def _toy_logits(seed=0):
    """a table model: the next token's logits are a fixed function of the whole prefix"""
    g = torch.Generator().manual_seed(seed)
    table = {}

    def row(prefix):
        key = tuple(prefix)
        if key not in table:
            table[key] = 2.0 * torch.randn(V5, generator=g, dtype=torch.float64)
        return table[key]

    # rows are created in the order they are asked for: fix that order (all prefixes, shortest first), whoever asks first
    for n in range(STEPS5):
        for key in itertools.product(range(V5), repeat=n):
            row(key)
    return lambda prefixes: torch.stack([row(p) for p in prefixes])


def _enumerate(logits_fn):
    """every hypothesis of at most STEPS5 tokens that ends at its first [STOP] or at STEPS5 tokens, with its log-probability"""
    out = []

    def walk(prefix, score):
        if len(prefix) == STEPS5 or (prefix and prefix[-1] == STOP5):
            out.append((score, prefix))
            return
        logp = torch.log_softmax(logits_fn([prefix])[0], -1).tolist()
        for t in range(V5):
            walk(prefix + [t], score + logp[t])
    walk([], 0.0)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_is_exact_when_the_beam_holds_every_prefix(seed):
    """V = 5, 4 steps, W = 125 = 5 ** 3: nothing is ever pruned before the last step, so the result is the 125 most likely of ALL
    hypotheses, which exhaustive enumeration gives."""
    fn = _toy_logits(seed)
    hyps, trace = beam_util.beam_search(fn, 125, STEPS5, STOP5, pad_token=0)
    every = sorted(_enumerate(fn), key=lambda x: -x[0])
    assert len(every) > 125 and len(hyps) == 125 and len(trace) == STEPS5
    for (toks, score, length, fin), (want_score, want) in zip(hyps, every[:125]):
        assert toks[:length] == want and all(t == 0 for t in toks[length:]), (toks, want)
        assert abs(score - want_score) < 1e-12
        assert length == len(want) and fin == (want[-1] == STOP5)
    assert [h[1] for h in hyps] == sorted((h[1] for h in hyps), reverse=True)


def test_restatement_on_a_hand_worked_case():
    """W = 2, tokens 0 = pad, 1 = [STOP], 2, 3.  Step 1: P(2) = .5, P(3) = .4, P([STOP]) = .1 -> beams [2], [3].  Step 2: behind [2]
    P = (.3, .3, .4) for ([STOP], 2, 3), behind [3] P([STOP]) = .9 -> [3, STOP] = .36 (finished) and [2, 3] = .20: the greedy path
    [2, 3] is NOT the most likely one.  Step 3: [3, STOP] continues as itself, behind [2, 3] P([STOP]) = .5 -> [2, 3, STOP] = .10."""
    table = {(): [0, .1, .5, .4], (2,): [0, .3, .3, .4], (3,): [0, .9, .05, .05], (2, 3): [0, .5, .25, .25]}
    fn = lambda prefixes: torch.tensor([table.get(tuple(p), [.25] * 4) for p in prefixes], dtype=torch.float64).log()   # noqa: E731  (finished rows: unread)
    hyps, trace = beam_util.beam_search(fn, 2, 5, stop_token=1, pad_token=0)
    assert len(trace) == 3                                      # every hypothesis finished: the search ends
    assert [(p, t) for _, p, t in trace[0][0]] == [(0, 2), (0, 3)]
    assert [(p, t) for _, p, t in trace[1][0]] == [(1, 1), (0, 3)]
    assert [(p, t) for _, p, t in trace[2][0]] == [(0, 0), (1, 1)]
    assert abs(trace[1][1] - (math.log(.20) - math.log(.15))) < 1e-12          # [2, 3] against [2, STOP] (parent 0, token 1)
    (t0, s0, n0, f0), (t1, s1, n1, f1) = hyps
    assert t0 == [3, 1, 0] and n0 == 2 and f0 and abs(s0 - math.log(.36)) < 1e-12
    assert t1 == [2, 3, 1] and n1 == 3 and f1 and abs(s1 - math.log(.10)) < 1e-12


def test_restatement_tie_and_finished_rules():
    logits = torch.zeros(2, 6, dtype=torch.float64)
    logits[0, 4] = logits[0, 2] = 3.0                           # two equal logits in one row: the smaller token first
    logits[1] = logits[0]                                       # two identical rows with equal cum: the smaller parent first
    best, gap = beam_util.select(logits, [-1.0, -1.0], [False, False], 3, 0)
    assert [(p, t) for _, p, t in best] == [(0, 2), (0, 4), (1, 2)] and gap == 0.0
    best, _ = beam_util.select(logits, [-1.0, -2.0], [True, True], 2, 0)          # all finished: the group reproduces itself
    assert best == [(-1.0, 0, 0), (-2.0, 1, 0)]
    assert beam_util.merge(best, [True, True], [3, 5], 1) == ([-1.0, -2.0], [True, True], [3, 5])
    best, _ = beam_util.select(logits, [0.0, float("-inf")], [False, False], 2, 0)   # the first step: row 0 alone contributes
    assert [(p, t) for _, p, t in best] == [(0, 2), (0, 4)]
