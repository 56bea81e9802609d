"""Guided optimisation in the embedding space: gradient ascent on a property head's prediction, held near its start by an anchor and
pushed out of visited places by Gaussian hills (the "metadynamics" use the reference's README names; its notebook is not part of the
reference checkout, so the optimiser is this project's own and is pinned by the float64 restatement in tests/test_guide_cpu.py).

The property term and its gradient come from one kernel call per step for all trajectories together (PropertyHead.value_and_grad:
coati_head_grad, include/coati_guide.h); the anchor and hill terms are plain torch.

A GPHead has P means and one shared variance and no gradient of its own; its acquisition (mean, ucb, lcb or expected improvement of one
output: GPHead.acquisition, one coati_head_gp_grad call per step, include/coati_acq.h) is an objective this loop takes as it takes a head:

    guided_ascent(start, gp.acquisition("lcb", beta=2.0), steps=..., anchor=...)"""
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

from . import coati_purifications as _P

MAX_CENTRES = 64


@dataclass
class GuidedResult:
    vectors: torch.Tensor      # [n, dim] where the trajectories ended
    values: torch.Tensor       # [n, P] the head on them
    history: torch.Tensor      # [steps + 1, n] the objective's property term w . head(v) before every step and after the last
    centres: torch.Tensor      # [n, 64, dim] every trajectory's own hill centres, of which the first n_centres are set
    n_centres: int


def _weights(weights, P, like):
    w = torch.ones(P) if weights is None else torch.as_tensor(weights)
    if w.dim() != 1 or w.shape[0] != P:
        raise ValueError(f"guided_ascent: weights must be [{P}], got {tuple(w.shape)}")
    return w.to(device=like.device, dtype=like.dtype)


def guided_ascent(start, head, weights=None, steps=100, lr=0.05, anchor=0.0, bump_every=0, bump_height=1.0, bump_width=1.0, max_step=None,
                  value_and_grad: Optional[Callable] = None) -> GuidedResult:
    """n trajectories from the rows of start [n, dim], advanced together for `steps` steps of v <- v + lr * grad J_i(v) on

        J_i(v) = w . head(v) - anchor * |v - start_i|^2 - sum_m bump_height * exp(-|v - c_im|^2 / (2 bump_width^2)).

    Before step t (t = bump_every, 2 bump_every, ... < steps) the current v_i becomes one more centre c_im of trajectory i's own hills;
    bump_every = 0: no hills.  A trajectory holds at most 64 centres: more is a ValueError before the first step.  max_step: a step
    longer than that (Euclidean, per row) is scaled down to it.  weights: [P], default ones.  Deterministic.

    value_and_grad(vectors, cotangent [P]) -> (values [n, P], grad [n, dim] of cotangent . values): default head.value_and_grad, the
    kernel; any callable of that contract (an autograd-backed one, say) runs the same loop elsewhere."""
    steps, bump_every = int(steps), int(bump_every)
    if steps < 0 or bump_every < 0:
        raise ValueError(f"guided_ascent: steps={steps} and bump_every={bump_every} must not be negative")
    n_hills = (steps - 1) // bump_every if bump_every and steps > 0 else 0
    if n_hills > MAX_CENTRES:
        raise ValueError(f"guided_ascent: steps={steps} with bump_every={bump_every} would set {n_hills} centres per trajectory; "
                         f"at most {MAX_CENTRES} are kept")
    if bump_every and float(bump_width) <= 0.0:
        raise ValueError(f"guided_ascent: bump_width={bump_width} must be positive")
    start = torch.as_tensor(start)
    if start.dim() == 1:
        start = start[None]
    if start.dim() != 2 or not start.is_floating_point():
        raise ValueError(f"guided_ascent: start must be a float tensor [n, dim], got {tuple(start.shape)}")
    if value_and_grad is None:
        if getattr(head, "has_input_gradient", True) is False:
            raise TypeError(f"guided_ascent: a {type(head).__name__} has no gradient with respect to the embedding (uncertainty-aware ascent "
                            "is not implemented); climb its extractor (head.extractor) or pass value_and_grad=")
        value_and_grad = head.value_and_grad
        start = start.to(head.device)
    start = start.detach()
    P = int(head.num_outputs)
    w = _weights(weights, P, start)
    n, dim = start.shape
    v = start.clone()
    centres = torch.zeros(n, MAX_CENTRES, dim, dtype=start.dtype, device=start.device)
    count = 0
    history = []
    with torch.no_grad():
        for t in range(steps):
            if bump_every and t > 0 and t % bump_every == 0:
                centres[:, count] = v
                count += 1
            values, grad = value_and_grad(v, w)
            values, grad = values.to(v), grad.to(v)
            history.append((values * w).sum(dim=1))
            if float(anchor) != 0.0:
                grad = grad - 2.0 * float(anchor) * (v - start)
            if count:
                diff = v[:, None, :] - centres[:, :count]                                        # [n, count, dim]
                hill = float(bump_height) * torch.exp(-(diff * diff).sum(dim=2) / (2.0 * float(bump_width) ** 2))
                grad = grad + (hill[:, :, None] * diff).sum(dim=1) / float(bump_width) ** 2
            step = lr * grad
            if max_step is not None:
                length = step.norm(dim=1, keepdim=True)
                step = step * torch.clamp(float(max_step) / length.clamp_min(1e-30), max=1.0)
            v = v + step
        values, _ = value_and_grad(v, w)
        values = values.to(v)
        history.append((values * w).sum(dim=1))
    return GuidedResult(v, values, torch.stack(history), centres, count)


def guided_generation(smiles_or_vectors, head, encoder, tokenizer, weights=None, steps=100, lr=0.05, anchor=0.0, bump_every=0, bump_height=1.0,
                      bump_width=1.0, max_step=None, grammar=None, canon_smiles=None, generator=None, decode: Optional[Callable] = None,
                      embed: Optional[Callable] = None, value_and_grad: Optional[Callable] = None) -> List[Dict]:
    """Molecules from guided_ascent: the starts (SMILES strings, embedded; or vectors [n, dim]) are optimised, the end points decoded
    together (decode(vectors) -> strings; default force_decode_valid_batches, grammar= passed through), what decoded to a usable string
    (a non-empty str) is embedded again (embed(strings) -> [n, dim]; default embed_smiles_batch) and scored with head.predict: a decoded
    molecule is not the vector it came from.  Returns [{"start", "smiles", "start_value", "vector_value", "decoded_value"}] ordered by
    decoded_value, best first (ties: start order); the values are w . head(.), start is the start's string, or its row number when
    vectors were given.  A start whose end point does not decode is dropped."""
    if decode is None:
        def decode(V):
            return _P.force_decode_valid_batches(V, encoder, tokenizer, canon_smiles=canon_smiles, generator=generator, grammar=grammar)
    if embed is None:
        def embed(strings):
            return _P.embed_smiles_batch(strings, encoder, tokenizer)
    if isinstance(smiles_or_vectors, (list, tuple)) and all(isinstance(s, str) for s in smiles_or_vectors):
        names = list(smiles_or_vectors)
        start = embed(names)
    else:
        start = torch.as_tensor(smiles_or_vectors)
        if start.dim() == 1:
            start = start[None]
        names = list(range(start.shape[0]))
    res = guided_ascent(start, head, weights=weights, steps=steps, lr=lr, anchor=anchor, bump_every=bump_every, bump_height=bump_height,
                        bump_width=bump_width, max_step=max_step, value_and_grad=value_and_grad)
    decoded = list(decode(res.vectors))
    kept = [i for i, s in enumerate(decoded) if isinstance(s, str) and s]
    if not kept:
        return []
    with torch.no_grad():
        again = head.predict(embed([decoded[i] for i in kept]))
        w = _weights(weights, int(head.num_outputs), again)
        decoded_value = (again * w).sum(dim=1).cpu().tolist()
    first, last = res.history[0].cpu().tolist(), res.history[-1].cpu().tolist()
    records = [{"start": names[i], "smiles": decoded[i], "start_value": first[i], "vector_value": last[i], "decoded_value": dv}
               for i, dv in zip(kept, decoded_value)]
    records.sort(key=lambda r: -r["decoded_value"])
    return records
