"""Shared by the guided-optimisation tests (test_guide_cpu.py, test_gpu_guide.py): a restatement of coati_head_grad's arithmetic with its
masks exposed and its K sums optionally chunked, heads whose forward is exact but whose backward is not, cotangents, an autograd-backed
value_and_grad, and the C entry called on raw tensors.  Builds on screen_util, which stays as it is."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import screen_util as U  # noqa: E402

from coati_amd.models.regression import PropertyHead  # noqa: E402

EXACT_SHAPES = [(32, 64, 0, 1), (32, 64, 1, 1), (64, 128, 3, 8), (256, 256, 4, 1), (512, 256, 2, 3)]
RANDOM_SHAPES = [(256, 256, 4, 1), (256, 128, 4, 2), (512, 256, 8, 3), (32, 64, 1, 1)]
TERNARY_SHAPES = [(256, 256, 4, 1), (256, 128, 4, 2), (512, 256, 8, 3), (32, 64, 1, 1), (64, 128, 16, 8)]


def restate(head, x16, cot, dtype=torch.float64, chunks=1):
    """(out, g, masks) of PropertyHead.reference_grad's arithmetic in `dtype`, every product's K sum taken in `chunks` pieces that are then
    added in `dtype` (chunks = 1: one piece, reference_grad itself); masks [D, n, F] are the ReLU decisions"""
    def rb(t):
        return t.detach().to(torch.float32).to(torch.bfloat16).to(dtype)

    def mm(a, w):                       # a [n, K] . w [M, K]^T
        K = a.shape[1]
        step = max(1, K // chunks)
        acc = None
        for lo in range(0, K, step):
            part = a[:, lo:lo + step] @ w[:, lo:lo + step].T
            acc = part if acc is None else acc + part
        return acc

    with torch.no_grad():
        w0 = rb(head.first.weight)
        wr = [rb(res.weight) for res in head.residuals]
        wl = head.last.weight.detach().to(dtype)
        h = mm(x16[:, :head.input_dim].to(dtype), w0) + head.first.bias.to(dtype)
        masks = []
        for res, w in zip(head.residuals, wr):
            z = mm(rb(h), w) + res.bias.to(dtype)
            masks.append(z > 0)
            h = h + torch.relu(z)
        out = mm(h, wl) + head.last.bias.to(dtype)
        d = mm(cot.to(dtype), wl.T.contiguous())
        for m, w in zip(reversed(masks), reversed(wr)):
            d = d + mm(rb(torch.where(m, d, torch.zeros_like(d))), w.T.contiguous())
        g = mm(rb(d), w0.T.contiguous())
        g = torch.nn.functional.pad(g, (0, x16.shape[1] - head.input_dim))
        return out, g, (torch.stack(masks) if masks else torch.zeros(0, x16.shape[0], head.features, dtype=torch.bool))


def exact_cot(n, P, seed):
    """cotangents from {+-0.5, +-1}: nothing is zeroed, every product stays exact"""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (n, P), generator=g)]


def ternary_head(E, F, D, P, seed):
    """A head whose forward sums are exact in any order and whose backward is ordinary f32 arithmetic: first and residual weights are dense
    ternary (a random sign where randint(0, 8) == 0, else 0), scaled by 0.5 (first) and 0.25 (residual), biases multiples of 0.5 in
    [-1, 1]; last.weight and last.bias unit Gaussian."""
    g = torch.Generator().manual_seed(seed)
    head = PropertyHead(E, features=F, depth=D, num_outputs=P)

    def ternary(rows, cols):
        on = (torch.randint(0, 8, (rows, cols), generator=g) == 0).float()
        return on * (torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1)

    def half_steps(k):
        return torch.randint(-2, 3, (k,), generator=g).float() * 0.5

    with torch.no_grad():
        head.first.weight.copy_(0.5 * ternary(F, E))
        head.first.bias.copy_(half_steps(F))
        for res in head.residuals:
            res.weight.copy_(0.25 * ternary(F, F))
            res.bias.copy_(half_steps(F))
        head.last.weight.copy_(torch.randn(P, F, generator=g))
        head.last.bias.copy_(torch.randn(P, generator=g))
    return head


def row_error(g, ref):
    """per row: max |g - ref| / max |ref| over the whole of ref"""
    return (g.double() - ref).abs().max(dim=1).values / float(ref.abs().max())


def autograd_value_and_grad(head):
    """a value_and_grad of PropertyHead.value_and_grad's contract from autograd through head.forward, in the vectors' dtype"""
    def fn(v, cot):
        with torch.enable_grad():
            x = v.detach().clone().requires_grad_(True)
            values = head(x)
            (grad,) = torch.autograd.grad((values * cot.to(values)).sum(), x)
        return values.detach(), grad
    return fn


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def head_grad_raw(head, x16, cot, out, g, n, ldx=None, ldc=None, ldo=None, ldg=None):
    """coati_head_grad on tensors as they lie: the first n rows of x16, cot, out and g at their own row strides"""
    from coati_amd import _lib
    w0, b0, wr, br, wl, bl = head._operands()
    w0t, wrt = head._grad_operands()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("coati_head_grad", _ptr(x16), x16.stride(0) if ldx is None else ldx, n, head.input_dim_padded, _ptr(w0), _ptr(b0), _ptr(wr),
              _ptr(br), head.depth, _ptr(wl), _ptr(bl), head.num_outputs, head.features, _ptr(w0t), _ptr(wrt), _ptr(cot),
              cot.stride(0) if ldc is None else ldc, _ptr(out), out.stride(0) if ldo is None else ldo, _ptr(g),
              g.stride(0) if ldg is None else ldg, stream)
