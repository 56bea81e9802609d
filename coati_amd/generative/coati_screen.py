"""A filtered virtual screen over samples of an embedding-space distribution (the reference's generation_examples notebook routine),
batched: the samples of a batch that a property head scores above the threshold are decoded together, re-embedded together and scored
again, and those still above it are kept.  The head is a coati_amd.models.regression.PropertyHead (its predict() is one fused kernel)."""
from typing import Callable, Dict, List, Optional

import torch

from . import coati_purifications as _P


def sampled_virtual_screen(sample_maker, head, encoder, tokenizer, hit_thresh, n_to_draw: int = 15, batch_size: int = 512, output: int = 0,
                           max_batches: int = 100, canon_smiles=None, generator=None, grammar=None,
                           decode: Optional[Callable] = None, embed: Optional[Callable] = None, beta: float = 0.0) -> List[Dict]:
    """Draws sample_maker.rsample([batch_size]) until n_to_draw molecules are found or max_batches batches are spent.  Of each batch
    the vectors with head.predict(vectors)[:, output] > hit_thresh are decoded to valid SMILES (decode(vectors) -> strings; default
    force_decode_valid_batches), the strings embedded (embed(strings) -> [n, E]; default embed_smiles_batch) and scored again: a decoded
    molecule is not the vector it came from.  Returns [{"smiles", "score"}] of those still above the threshold, in the order found, at
    most n_to_draw of them (the notebook's loop finishes its batch and may return more).

    beta > 0: the head must offer predict_with_std (a GPHead); both filters apply the threshold to mean - beta * std, a prediction the head
    is unsure of has to be that much better, and the records gain "std" ("score" stays the mean)."""
    beta = float(beta)
    if beta < 0.0:
        raise ValueError(f"sampled_virtual_screen: beta={beta} must not be negative")
    if beta > 0.0 and not hasattr(head, "predict_with_std"):
        raise TypeError("sampled_virtual_screen: beta > 0 needs a head with predict_with_std (a GPHead)")
    if decode is None:
        def decode(V):
            return _P.force_decode_valid_batches(V, encoder, tokenizer, canon_smiles=canon_smiles, generator=generator, grammar=grammar)
    if embed is None:
        def embed(strings):
            return _P.embed_smiles_batch(strings, encoder, tokenizer)
    history: List[Dict] = []
    with torch.no_grad():
        for _ in range(int(max_batches)):
            if len(history) >= n_to_draw:
                break
            vecs = sample_maker.rsample([batch_size])
            if beta > 0.0:
                mean, std = head.predict_with_std(vecs)
                good = vecs[(mean[:, output] - beta * std[:, output] > hit_thresh).to(vecs.device)]
                if good.shape[0] == 0:
                    continue
                smiles = list(decode(good))
                mean, std = head.predict_with_std(embed(smiles))
                scores, stds = mean[:, output].cpu().tolist(), std[:, output].cpu().tolist()
                for s, score, sd in zip(smiles, scores, stds):
                    if score - beta * sd > hit_thresh and len(history) < n_to_draw:
                        history.append({"smiles": s, "score": score, "std": sd})
                continue
            first = head.predict(vecs)[:, output]
            good = vecs[(first > hit_thresh).to(vecs.device)]
            if good.shape[0] == 0:
                continue
            smiles = list(decode(good))
            scores = head.predict(embed(smiles))[:, output].cpu().tolist()
            for s, score in zip(smiles, scores):
                if score > hit_thresh and len(history) < n_to_draw:
                    history.append({"smiles": s, "score": score})
    return history
