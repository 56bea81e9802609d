"""Shared by the property-head tests (test_screen_cpu.py, test_gpu_screen.py): heads whose every sum is exact, f32 restatements of the
kernel's arithmetic in two summation orders, and the C entry called on raw tensors."""
import ctypes

import torch

from coati_amd.models.regression import PropertyHead


def exact_head(E, F, D, P, seed, unit_input=False):
    """A head all of whose arithmetic is exact in any order: first and every residual weight have one +-1 per row (a random column) and,
    in one row of four, one extra +-0.5; biases are multiples of 0.5 in [-1, 1]; last has small integers.  With inputs in {-2 .. 2}
    every value of the stream is a multiple of 2^-(D + 1) of modest size: any row, column, K slab or layer mixed up gives a wrong value."""
    g = torch.Generator().manual_seed(seed)
    head = PropertyHead(E, features=F, depth=D, num_outputs=P, unit_input=unit_input)

    def signed_perm(rows, cols):
        w = torch.zeros(rows, cols)
        r = torch.arange(rows)
        c = torch.randint(0, cols, (rows,), generator=g)
        w[r, c] = torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1
        c2 = (c + 1 + torch.randint(0, cols - 1, (rows,), generator=g)) % cols          # another column
        extra = (torch.randint(0, 2, (rows,), generator=g).float() - 0.5) * (torch.randint(0, 4, (rows,), generator=g) == 0).float()
        w[r, c2] = extra
        return w

    def half_steps(n):
        return torch.randint(-2, 3, (n,), generator=g).float() * 0.5

    with torch.no_grad():
        head.first.weight.copy_(signed_perm(F, E))
        head.first.bias.copy_(half_steps(F))
        for res in head.residuals:
            res.weight.copy_(signed_perm(F, F))
            res.bias.copy_(half_steps(F))
        head.last.weight.copy_(torch.randint(-3, 4, (P, F), generator=g).float())
        head.last.bias.copy_(half_steps(P))
    return head


def exact_rows(n, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n, E), generator=g).to(torch.bfloat16)


def unrounded(head, x16, dtype=torch.float64):
    """reference() without the bf16 rounding of the stream: forward on the rows as they are, in dtype"""
    with torch.no_grad():
        h = x16[:, :head.input_dim].to(dtype) @ head.first.weight.to(dtype).T + head.first.bias.to(dtype)
        for res in head.residuals:
            h = h + torch.relu(h @ res.weight.to(dtype).T + res.bias.to(dtype))
        return h @ head.last.weight.to(dtype).T + head.last.bias.to(dtype)


def restate_f32_chunked(head, x16, chunks=8):
    """reference(x16, float32) with every product's K sum taken in `chunks` pieces that are then added in f32: another summation order"""
    def rb(t):
        return t.detach().to(torch.bfloat16).float()

    def mm(a, w):
        K = a.shape[1]
        step = max(1, K // chunks)
        acc = None
        for lo in range(0, K, step):
            part = a[:, lo:lo + step] @ w[:, lo:lo + step].T
            acc = part if acc is None else acc + part
        return acc

    with torch.no_grad():
        h = mm(x16[:, :head.input_dim].float(), rb(head.first.weight)) + head.first.bias
        for res in head.residuals:
            h = h + torch.relu(mm(rb(h), rb(res.weight)) + res.bias)
        return mm(h, head.last.weight.float()) + head.last.bias


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def head_eval_raw(head, x16, out, n, ldx=None, ldo=None):
    """coati_head_eval on tensors as they lie: x16's first n rows at stride ldx, out at row stride ldo"""
    from coati_amd import _lib
    w0, b0, wr, br, wl, bl = head._operands()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("coati_head_eval", _ptr(x16), x16.stride(0) if ldx is None else ldx, n, head.input_dim_padded, _ptr(w0), _ptr(b0), _ptr(wr),
              _ptr(br), head.depth, _ptr(wl), _ptr(bl), head.num_outputs, head.features, _ptr(out),
              out.stride(0) if ldo is None else ldo, stream)
