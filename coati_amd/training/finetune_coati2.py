"""Fine-tuning a COATI2 model on SMILES: the autoregressive loss of [CLIP][UNK][SMILES] (+ [SUFFIX][MIDDLE]) <smi>[STOP] under
coati_to_token(smiles_to_coati(encoder pass over [SMILES]<smi>[STOP])) at [UNK] -- the rows batch_smiles_to_s2s_likelihood scores --,
clip-norm and AdamW, on the engine's training step (Engine.train_step on a COATI2 layout, packed rows)."""
import random
from typing import List

import torch

from ..models.encoding.clip_e2e import s2s_hcoati_likelihood_tokens
from ..synthetic import packed_lengths


def finetune_coati2(model, tokenizer, smiles: List[str], n_steps: int, batch_size: int, lr: float, do_suffix: bool = False, rng=None,
                    **opt_kw) -> List[float]:
    """n_steps optimiser steps of `model` (COATI_Smiles_Inference(..., trainable=True) / load_coati2(..., trainable=True)) on batches of
    batch_size strings drawn without replacement from `smiles` by `rng` (a random.Random; default seed 0).  Strings that do not tokenize
    or do not fit n_seq are dropped from their batch; a batch of which nothing is left is skipped (its loss: nan).  opt_kw: weight_decay /
    max_norm / betas / eps of Engine.optimizer_step.  Returns the AR loss (mean NLL per target token) of every step, before its update."""
    if not getattr(model, "trainable", False):
        raise ValueError("finetune_coati2: the model was built with trainable=False (no gradient or Adam buffers)")
    model._sync_tokens(tokenizer)
    eng = model.engine
    rng = rng or random.Random(0)
    smiles = list(smiles)
    losses = []
    for _ in range(int(n_steps)):
        picked = rng.sample(smiles, min(int(batch_size), len(smiles)))
        raw, tokens, y_next, mask = s2s_hcoati_likelihood_tokens(picked, tokenizer, do_suffix)
        if not bool(mask.any()):
            losses.append(float("nan"))
            continue
        l_raw, l_tok = packed_lengths(raw, tokens, y_next, pad=eng.cfg.pad_token)
        batch = {"raw_tokens": raw.to(eng.device).contiguous(), "tokens": tokens.to(eng.device).contiguous(),
                 "y_next": y_next.to(eng.device).contiguous(), "rows": (int(l_raw.sum()), int(l_tok.sum()))}
        eng.train_step(batch, None, lr, do_clip=False, **opt_kw)
        losses.append(eng.losses()["ar_loss"])
    return losses
