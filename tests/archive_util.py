"""The archive rule restated for the tests (rogue-gym_amd/csrc/rg_archive.h is the product's statement; nothing here shares code with it): a Python dict keyed
by the cell that keeps the best offer's score, steps, call and record bytes and knows nothing of slots or probing; for the overflow tests only, which keys a
table of given occupancy still has room for; and the host entry's table."""
import ctypes as C

import numpy as np

PROBES = 1024
I32_MIN, I32_MAX, U32_MAX = -(1 << 31), (1 << 31) - 1, (1 << 32) - 1
SLOT = np.dtype([("key", "<u8"), ("score", "<i4"), ("steps", "<u4"), ("seen", "<u4"), ("chosen", "<u4"), ("when", "<u4"), ("zero", "<u4")])


def beats(score_a, steps_a, score_b, steps_b):
    return score_a > score_b or (score_a == score_b and steps_a < steps_b)


class DictArchive:
    """cell -> [score, steps, seen, when, record]: the oracle.  One update() is one call: every offer counts as seen; the call's best offer (ties: the lowest
    env) replaces the stored one only if it beats it strictly."""

    def __init__(self):
        self.cells, self.calls, self.replaced, self.offers = {}, 0, 0, 0

    def update(self, keys, scores, steps, records=None, envs=None, admit=None):
        """keys / scores / steps indexed by env; records [N, R] or None; envs: those that offer (default all); admit(key) -> bool: whether the table has room
        for the key (default: always).  Returns (stored bool [N], dropped bool [N])."""
        n = len(keys)
        envs = range(n) if envs is None else envs
        self.calls += 1
        stored, dropped = np.zeros(n, bool), np.zeros(n, bool)
        best = {}
        for e in envs:
            k = int(keys[e]) or 1
            if k not in self.cells and admit is not None and not admit(k):
                dropped[e] = True
                continue
            self.offers += 1
            c = self.cells.setdefault(k, [None, None, 0, 0, None])
            c[2] += 1
            b = best.get(k)
            if b is None or beats(int(scores[e]), int(steps[e]), int(scores[b]), int(steps[b])):
                best[k] = e
        for k, e in best.items():
            c = self.cells[k]
            if c[3] == 0 or beats(int(scores[e]), int(steps[e]), c[0], c[1]):
                self.replaced += c[3] != 0
                c[0], c[1], c[3] = int(scores[e]), int(steps[e]), self.calls
                c[4] = None if records is None else records[e].copy()
                stored[e] = True
        return stored, dropped

    def rows(self):
        """(keys u64, score, steps, seen, when) sorted by key."""
        ks = sorted(self.cells)
        col = lambda i: np.array([self.cells[k][i] for k in ks], np.int64)
        return np.array(ks, np.uint64), col(0), col(1), col(2), col(3)


def admitted_by(keys_after):
    """admit(key) from the device's slot occupancy AFTER a call (u64 [cells], 0 = empty): which of the new keys that competed for the last empty slots got
    one is the one thing scheduling decides, so the oracle is told -- a key is admitted iff it stands in the table."""
    have = set(int(k) for k in np.asarray(keys_after) if k)
    return lambda key: key in have


def window_full(keys_after, key, cells):
    """No empty slot within min(cells, 1 024) probes of key & (cells - 1): what must hold for a dropped key (slots never empty again, so also after the call)."""
    idx = ((key & (cells - 1)) + np.arange(min(cells, PROBES))) & (cells - 1)
    return bool((np.asarray(keys_after)[idx] != 0).all())


def device_table(arc):
    """The occupied slots of env.archive sorted by key: (slots, keys u64, score, steps, seen, when) as numpy."""
    key = arc.key.cpu().numpy().view(np.uint64)
    at = np.nonzero(key)[0]
    at = at[np.argsort(key[at], kind="stable")]
    g = lambda t: t.cpu().numpy()[at].astype(np.int64)
    return at, key[at], g(arc.score), g(arc.steps), g(arc.seen), g(arc.when)


# ---- the host entry ----
def host_table(cells):
    """cells zeroed slots (8-byte aligned: numpy's allocation) of rg_archive_offer_host's table."""
    return np.zeros(cells, SLOT)


def offer_host(lib, slots, key, score, steps, serial):
    slot, stored = C.c_int32(-7), C.c_int32(-7)
    rc = lib.rg_archive_offer_host(slots.ctypes.data, len(slots), key, score, steps, serial, C.byref(slot), C.byref(stored))
    return rc, slot.value, stored.value
