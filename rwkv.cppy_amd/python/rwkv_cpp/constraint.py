"""Byte-level DFA constraints for device-side generation (rwkv_mi355x_constraint).

A constraint is a table next [n_states, 256] of uint16 (DEAD = 0xFFFF: no transition) and accepting
[n_states]; tokens are byte strings, and a token is allowed in state q when walking its bytes from q
never dies.  walk and allowed_mask restate in integers what the kernels of constrain.hip compute;
from_choices builds the automaton of "answer with one of these strings"."""
from typing import List, Optional, Sequence

import numpy as np

DEAD = 0xFFFF


class Dfa:
    """What the dfa= argument of RWKVModel.sample / generate / generate_batch / generate_queue takes:
    next, accepting and start (one state for every row, or one per row).  A call leaves state (the
    rows' states afterwards: pass them as start to continue) and ended (0 not ended, 1 a stop token, 2
    no token was allowed) on the object, uint32 arrays of one entry per row."""

    def __init__(self, next, accepting, start=0):
        self.next = np.ascontiguousarray(next, dtype=np.uint16).reshape(-1, 256)
        self.accepting = np.ascontiguousarray(accepting, dtype=np.uint8)
        if self.accepting.shape != (self.next.shape[0],):
            raise ValueError('one accepting flag per state')
        self.start = start
        self.state: Optional[np.ndarray] = None
        self.ended: Optional[np.ndarray] = None


class ResidentDfa(Dfa):
    """A Dfa whose table is resident on the model's context (RWKVModel.set_constraint_table): it carries
    n_states and the start states and no arrays.  state and ended come back as for any Dfa."""

    def __init__(self, n_states: int, start=0):
        self.next = self.accepting = None
        self.n_states = int(n_states)
        self.start = start
        self.state = self.ended = None


def walk(next, q: int, data: bytes) -> int:
    """The state after the bytes of data from q, or DEAD."""
    for b in data:
        if q == DEAD:
            break
        q = int(next[q][b])
    return q


def allowed_mask(next, accepting, q: int, vocab: Sequence[bytes], stops=()) -> np.ndarray:
    """bool [len(vocab)]: token t is allowed in state q iff it has at least one byte and its walk from
    q does not die; a stop token is allowed iff accepting[q], whatever its bytes."""
    stops = set(int(t) for t in stops)
    return np.array([bool(accepting[q]) if t in stops else (len(v) > 0 and walk(next, q, v) != DEAD)
                     for t, v in enumerate(vocab)], dtype=bool)


def from_choices(choices: List[bytes]) -> Dfa:
    """The trie of the choices as a DFA: state 0 is the root, a state is accepting where a choice is
    complete (a choice may be a prefix of another)."""
    rows = [np.full(256, DEAD, np.uint16)]
    accepting = [0]
    for choice in choices:
        if len(choice) == 0:
            raise ValueError('an empty choice')
        q = 0
        for b in bytes(choice):
            if rows[q][b] == DEAD:
                rows[q][b] = len(rows)
                rows.append(np.full(256, DEAD, np.uint16))
                accepting.append(0)
            q = int(rows[q][b])
        accepting[q] = 1
    return Dfa(np.stack(rows), accepting)


def join(*dfas: Dfa):
    """Several automata as disjoint state sets of one table.  Returns (Dfa, [the start state of each])."""
    nexts, starts, base = [], [], 0
    for d in dfas:
        n = d.next.astype(np.uint32)
        nexts.append(np.where(n == DEAD, DEAD, n + base).astype(np.uint16))
        starts.append(base + int(np.atleast_1d(d.start)[0]))
        base += d.next.shape[0]
    return Dfa(np.concatenate(nexts), np.concatenate([d.accepting for d in dfas]), starts), starts


def pack_vocab(vocab: Sequence[bytes]):
    """(offsets uint32 [V + 1], bytes uint8) as rwkv_mi355x_vocab_bytes takes them."""
    offsets = np.zeros(len(vocab) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(v) for v in vocab])
    data = np.frombuffer(b''.join(bytes(v) for v in vocab) or b'\0', dtype=np.uint8)
    return offsets, np.ascontiguousarray(data)
