"""Syntax-constrained decoding: the automaton behind `grammar=` of the engine's decode paths (include/coati_grammar.h,
csrc/grammar.hip).  Plain Python, numpy and torch; importable without a GPU.

With a grammar every finished string has balanced parentheses, closed ring-bond digits and closed bracket atoms, and reaches [STOP]
on its own within n_seq.  The constraint is syntactic only: valence, aromaticity and empty branches stay rdkit's business.

The vocabulary's tokens are multi-symbol pieces (`c1ccccc1`, `(=O)c1`, `[C@@H](C)C`), so "may this token follow" is decided from a
per-row state and a per-token entry:

  state  (depth, rings, flags): open parentheses; bit d of rings = ring digit d is open (d = 0 .. 9); flags bit 0 = inside a bracket
         atom, bit 1 = dead, bit 2 = finished.  On the device four int32 per row, the fourth 0.
  cost(s) = depth + popcount(rings) + inbr: the single-symbol closers still owed.
  entry  8 bytes, table [2][V], first index = the bracket state the token is entered in:
         byte 0 need (the depth the token's prefix requires), byte 1 delta (int8, net change of depth), bytes 2-3 toggle (the ring
         digits the token flips), byte 4: bit 0 may be sampled from this state, bit 1 bracket state at the token's end, bit 2 neutral
         (a special token: never sampled; forced, it leaves the state alone).

An entry is built by scanning the token's text symbol by symbol from the entry state: `(` `)` `[` inside a bracket and `]` outside
one make it invalid; a digit outside a bracket flips its ring bit, inside one nothing (`[NH3+]`, `[13C]`); every other symbol is
neutral.  `%` makes the entry invalid: TWO-DIGIT RING CLOSURES (`%10` ..) ARE NOT GENERATED UNDER THE CONSTRAINT -- the id would span
tokens and make every digit token's meaning depend on a third state.  (How often drug-like sets need ring ids >= 10 is unmeasured
here.)  A forced token with an invalid entry (in a prompt) makes the row dead.

Admission, with R = the positions still to be drawn, the one being drawn included, in an alive, unfinished state s:
  [STOP]           iff cost(s) == 0
  any other token  iff it may be sampled from s.inbr, s.depth >= need and cost(s') <= R - 2   (room for the closers and [STOP]),
                   s' = (depth + delta, rings ^ toggle, the token's end bracket state)
Alive implies cost(s) <= R - 1, and the vocabulary holds `)`, `]` and `0` .. `9` as single tokens (from_tokenizer refuses one that
does not), so the admitted set is never empty: a closer lowers the cost by one, and at R = 1 only [STOP] is left.

Advance by a drawn or forced token: a finished or dead state stays; [STOP] finishes the row (dead if cost != 0); a neutral token
leaves the state alone; a token that may not be entered from the state makes the row dead; otherwise the state becomes s', dead if
cost(s') exceeds what the positions behind the token can close (cost(s') > R - 1, R counted behind the token, at least 1).  A dead row
is no longer constrained; the engine reports it in Engine.last_grammar_violations.

walk / admitted / advance below are the restatement the tests pin the kernel to; balanced() is a string-level check that knows
nothing about tokens."""
import numpy as np
import torch

INBR, DEAD, FINISHED = 1, 2, 4              # state flags
SAMPLE, END_INBR, NEUTRAL = 1, 2, 4         # entry flags (byte 4)
EMPTY = (0, 0, 0)

_POP = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)


def cost(state):
    depth, rings, flags = state
    return depth + int(_POP[rings & 0xffff]) + (flags & INBR)


def scan(text, inbr):
    """(need, delta, toggle, end bracket state) of a token's text entered in bracket state inbr, or None where it is invalid."""
    if not text:
        return None
    depth = low = toggle = 0
    for ch in text:
        if ch == "%":
            return None
        if inbr:
            if ch in "()[":
                return None
            if ch == "]":
                inbr = 0
        elif ch == "]":
            return None
        elif ch == "[":
            inbr = 1
        elif ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            low = min(low, depth)
        elif ch in "0123456789":
            toggle ^= 1 << int(ch)
    return -low, depth, toggle, inbr


def balanced(smiles, detail=False):
    """String level: parentheses balanced and never negative, ring digits (single digits outside bracket atoms) closed, bracket atoms
    closed and free of `(` `)` `[`, no `]` outside one, no `%`.  detail=True: (balanced, dead) -- dead = a symbol that no continuation
    can mend."""
    depth = rings = inbr = 0
    dead = False
    for ch in smiles:
        if ch == "%":
            dead = True
        elif inbr:
            if ch in "()[":
                dead = True
            elif ch == "]":
                inbr = 0
        elif ch == "]":
            dead = True
        elif ch == "[":
            inbr = 1
        elif ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            dead = dead or depth < 0
        elif ch in "0123456789":
            rings ^= 1 << int(ch)
        if dead:
            break
    ok = not dead and depth == 0 and rings == 0 and inbr == 0
    return (ok, dead) if detail else ok


class SmilesGrammar:
    """The table of a vocabulary.  need / delta / toggle / flags: integer arrays [2, V] (see the module docstring)."""

    def __init__(self, need, delta, toggle, flags, stop_token):
        self.need, self.delta, self.toggle, self.flags = (np.asarray(a, dtype=np.int64).reshape(2, -1) for a in (need, delta, toggle, flags))
        self.n_token = int(self.need.shape[1])
        self.stop_token = int(stop_token)
        if not 0 <= self.stop_token < self.n_token:
            raise ValueError(f"SmilesGrammar: stop_token {stop_token} outside 0 .. {self.n_token - 1}")
        if self.need.min() < 0 or self.need.max() > 255 or self.delta.min() < -128 or self.delta.max() > 127:
            raise ValueError("SmilesGrammar: a token's need (0 .. 255) or delta (-128 .. 127) does not fit its byte")
        if self.toggle.min() < 0 or self.toggle.max() > 0x3ff or self.flags.min() < 0 or self.flags.max() > 7:
            raise ValueError("SmilesGrammar: toggle masks ring digits 0 .. 9, flags are three bits")
        packed = self.need | ((self.delta & 0xff) << 8) | (self.toggle << 16) | (self.flags << 32)
        self.table = torch.from_numpy(packed.astype(np.int64)).contiguous()      # [2, V], the 8-byte entries (little-endian)
        self._dev = {}

    @classmethod
    def from_tokenizer(cls, tokenizer):
        """The grammar of a TrieTokenizer (COATI1's or COATI2's): special tokens are neutral, SMILES tokens are scanned."""
        keys = list(tokenizer.special_tokens) + list(tokenizer.smiles_tokens)
        n_special = len(tokenizer.special_tokens)
        smiles = set(tokenizer.smiles_tokens)
        lacking = [c for c in [")", "]"] + list("0123456789") if c not in smiles]
        if lacking:
            raise ValueError(f"SmilesGrammar: the vocabulary lacks the single-symbol tokens {lacking}; without them a state can be left "
                             "with no admitted token")
        V = len(keys)
        need, delta, toggle, flags = (np.zeros((2, V), dtype=np.int64) for _ in range(4))
        for t, text in enumerate(keys):
            for inbr in (0, 1):
                if t < n_special:
                    flags[inbr, t] = NEUTRAL
                    continue
                e = scan(text, inbr)
                if e is None:
                    continue
                if e[0] > 255 or not -128 <= e[1] <= 127:
                    raise ValueError(f"SmilesGrammar: token {text!r}: need {e[0]} / delta {e[1]} does not fit its byte")
                need[inbr, t], delta[inbr, t], toggle[inbr, t] = e[0], e[1], e[2]
                flags[inbr, t] = SAMPLE | (END_INBR if e[3] else 0)
        return cls(need, delta, toggle, flags, tokenizer.stop_token)

    def device_table(self, device):
        """The table on `device` (int64 [2, V]; kept)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.table.to(device).contiguous()
        return self._dev[key]

    def entry(self, token, inbr=0):
        """(need, delta, toggle, flags) of a token entered in bracket state inbr"""
        return tuple(int(a[inbr, token]) for a in (self.need, self.delta, self.toggle, self.flags))

    def advance(self, state, token, remaining=None):
        """The state behind `token`.  remaining = the positions still to be drawn behind it (None: no length budget)."""
        depth, rings, flags = state
        if flags & (DEAD | FINISHED):
            return state
        token = int(token)
        if token == self.stop_token:
            return depth, rings, flags | FINISHED | (DEAD if cost(state) else 0)
        if not 0 <= token < self.n_token:
            return state
        need, delta, toggle, fl = self.entry(token, flags & INBR)
        if fl & NEUTRAL:
            return state
        if not fl & SAMPLE or depth < need:
            return depth, rings, flags | DEAD
        new = (depth + delta, rings ^ toggle, (flags & ~INBR) | (1 if fl & END_INBR else 0))
        if remaining is not None and cost(new) > max(int(remaining), 1) - 1:
            new = (new[0], new[1], new[2] | DEAD)
        return new

    def walk(self, tokens, remaining=None, state=EMPTY):
        """The state behind a token sequence.  remaining = the positions still to be filled, the first token's included (None: no
        length budget)."""
        for i, t in enumerate(tokens):
            state = self.advance(state, t, None if remaining is None else int(remaining) - i - 1)
        return state

    def admitted(self, state, remaining):
        """bool [V]: the tokens that may be drawn in `state` with `remaining` positions to go, this one included.  A dead or finished
        state is not constrained: all True."""
        depth, rings, flags = state
        if flags & (DEAD | FINISHED):
            return np.ones(self.n_token, dtype=bool)
        b = flags & INBR
        fl = self.flags[b]
        after = depth + self.delta[b] + _POP[(rings ^ self.toggle[b]) & 0xffff] + ((fl & END_INBR) != 0)
        ok = ((fl & SAMPLE) != 0) & (depth >= self.need[b]) & (after <= int(remaining) - 2)
        ok[self.stop_token] = cost(state) == 0
        return ok

    # ---- device side ------------------------------------------------------------------------------------------------------
    def states(self, rows, device):
        """int32 [B, 4] on `device` from a list of (depth, rings, flags)"""
        return torch.tensor([[s[0], s[1], s[2], 0] for s in rows], dtype=torch.int32).reshape(-1, 4).to(device).contiguous()

    def step(self, logits, state_in, state_out, tok_prev=None, parent=None, remaining=1, stream=None):
        """coati_grammar_step on logits [B, >= V] f32 (rows of any stride, masked in place) and states int32 [B, 4]."""
        from . import _lib
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[1] >= self.n_token
        B = int(logits.shape[0])
        for s in (state_in, state_out):
            assert s.dtype == torch.int32 and s.shape == (B, 4) and s.is_contiguous() and s.device == logits.device
        assert tok_prev is None or (tok_prev.dtype == torch.long and tok_prev.shape == (B,) and tok_prev.is_contiguous())
        assert parent is None or (parent.dtype == torch.int32 and parent.shape == (B,) and parent.is_contiguous())
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        if stream is None:
            stream = torch.cuda.current_stream(logits.device).cuda_stream
        _lib.call("coati_grammar_step", p(logits), int(logits.stride(0)), B, self.n_token, p(self.device_table(logits.device)), p(state_in),
                  p(state_out), p(tok_prev), p(parent), int(remaining), self.stop_token, stream)
