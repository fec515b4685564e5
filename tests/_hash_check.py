"""The shared checker of the hash-map tests: runs operation batches, one launch
per batch, on a map driver and judges every one of them against the
dictionary model (_hash_model.HashModel). Integers and bytes only: nothing is
sampled and nothing has a tolerance.

A driver is anything with the methods of tests/test_hash_model_gpu.py's
DeviceMap (numpy in, numpy out). test_hash_model_cpu.py runs the checker on a
plain-Python driver, right and deliberately wrong, so that the checker itself
is tested without a GPU.
"""
import numpy as np

from _hash_model import HashModel, KEY_HI, key_in_range

OK = 0


def _key(k):
    return tuple(int(c) for c in k)


def distinct_rows(rng, n, sizes):
    """One value row per occurrence and value array, all rows of one array
    distinct wherever its size allows (row = occurrence counter, then noise)."""
    out = []
    for sz in sizes:
        r = rng.integers(0, 256, size=(n, sz), dtype=np.uint8)
        tag = np.arange(n, dtype=np.uint64) + np.uint64(rng.integers(1 << 20))
        for b in range(min(sz, 4)):
            r[:, b] = ((tag >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(
                np.uint8)
        out.append(np.ascontiguousarray(r))
    return out


class Checker:
    def __init__(self, dev, value_sizes=(), model=None):
        self.dev = dev
        self.sizes = tuple(value_sizes)
        self.model = model or HashModel(dev.capacity(), self.sizes)
        assert dev.capacity() == self.model.capacity

    # -- Activate / Insert --------------------------------------------------
    def _judge_insert(self, keys, idx, mask, rows):
        keys = np.asarray(keys).reshape(-1, 3)
        m = self.model
        new = m.new_keys(keys)
        assert len(new) <= len(m.free), "test bug: batch exceeds the capacity"
        expect_zero = np.ones(len(keys), bool)
        winners = {}
        for k, pos in new.items():
            won = [p for p in pos if mask[p]]
            assert len(won) == 1, \
                "key %s: %d winners among %d occurrences" % (k, len(won),
                                                             len(pos))
            winners[k] = won[0]
            expect_zero[won[0]] = False
        assert not mask[expect_zero].any(), \
            "mask 1 for a present, duplicate or out-of-range key"
        assert not idx[expect_zero].any(), "losers must report index 0"
        widx = [int(idx[p]) for p in winners.values()]
        assert len(set(widx)) == len(widx), "winners share a buffer index"
        assert all(0 <= i < m.capacity for i in widx)
        assert set(widx) <= m.free, "a live buffer index was handed out"
        kb = self.dev.key_buffer()
        vb = [self.dev.value_buffer(j) for j in range(len(self.sizes))]
        for k, p in winners.items():
            i = int(idx[p])
            assert _key(kb[i]) == k, "key_buffer[%d] is not %s" % (i, k)
            if rows is not None:
                for j in range(len(self.sizes)):
                    assert vb[j][i].tobytes() == rows[j][p].tobytes(), \
                        "value %d of key %s is not the winner's row" % (j, k)
            # Activate writes no row: whatever the buffer holds is now the
            # key's value and must stay attached to it.
            m.commit_insert(k, i, [v[i].tobytes() for v in vb])
        if m.pristine:
            assert m.active() == set(range(m.size())), \
                "a fresh or cleared map hands out 0..m-1"

    def activate(self, keys, size=True):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        idx, mask = self.dev.activate(keys)
        self._judge_insert(keys, idx, mask, None)
        self.census(size)

    def insert(self, keys, rows, size=True):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        idx, mask = self.dev.insert(keys, rows)
        self._judge_insert(keys, idx, mask, rows if self.sizes else None)
        self.census(size)

    # -- Find ---------------------------------------------------------------
    def find(self, keys):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        idx, mask = self.dev.find(keys)
        want_m, want_i = self.model.find(keys)
        assert np.array_equal(mask, want_m), "find: membership differs"
        assert np.array_equal(idx.astype(np.int64), want_i), \
            "find: index differs (absent keys report 0)"

    # -- Erase --------------------------------------------------------------
    def erase(self, keys, size=True):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        mask = self.dev.erase(keys)
        present = self.model.present_keys(keys)
        expect_zero = np.ones(len(keys), bool)
        for k, pos in present.items():
            won = [p for p in pos if mask[p]]
            assert len(won) == 1, \
                "erase of %s: %d of %d occurrences succeeded" % (k, len(won),
                                                                 len(pos))
            expect_zero[won[0]] = False
        assert not mask[expect_zero].any(), \
            "erase succeeded for an absent or out-of-range key"
        for k in present:
            self.model.commit_erase(k)
        self.census(size)

    # -- Size and active indices --------------------------------------------
    def census(self, size=True):
        """`size=False` leaves o3dmi_hash_size out: it is the call that
        rebuilds a crowded table, and some scenarios need the table as it is."""
        act = self.dev.active()
        assert len(act) == self.model.size(), \
            "active_indices count %d, model %d" % (len(act),
                                                   self.model.size())
        assert set(int(i) for i in act) == self.model.active()
        if size:
            st, n = self.dev.size()
            assert st == OK, "size: status %d" % st
            assert n == self.model.size(), (n, self.model.size())

    # -- key -> index -> rows, re-read through find ---------------------------
    def association(self, same_indices=True):
        m = self.model
        keys = list(m.entries)
        if not keys:
            return {}
        idx, mask = self.dev.find(np.array(keys, np.int32).reshape(-1, 3))
        assert mask.all(), "a live key is not found"
        kb = self.dev.key_buffer()
        vb = [self.dev.value_buffer(j) for j in range(len(self.sizes))]
        out = {}
        for k, i in zip(keys, idx):
            i = int(i)
            if same_indices:
                assert i == m.entries[k][0], "key %s moved to %d" % (k, i)
            assert _key(kb[i]) == k
            for j in range(len(self.sizes)):
                assert vb[j][i].tobytes() == m.entries[k][1][j], \
                    "value %d of key %s changed" % (j, k)
            out[k] = i
        return out

    # -- Reserve / Clear / To -----------------------------------------------
    def reserve(self, capacity):
        m = self.model
        before = self.dev.capacity()
        st = self.dev.reserve(capacity)
        assert st == OK, "reserve: status %d" % st
        if capacity <= m.size():
            assert self.dev.capacity() == before, "this reserve is a no-op"
            self.association()
        else:
            assert self.dev.capacity() == capacity
            m.capacity = capacity    # for the bounds inside reindex
            m.reindex(capacity, self.association(same_indices=False))
            # re-inserted into a cleared table: the identity heap again
            assert m.active() == set(range(m.size()))
            m.pristine = True
        self.census()

    def clear(self):
        self.dev.clear()
        self.model.clear()
        self.census()

    def to_device(self):
        """A Checker on the copy; the source is checked to be unchanged."""
        other = self.dev.to_device()
        assert other.capacity() == self.dev.capacity()
        c = Checker(other, self.sizes, self.model.copy())
        c.model.reindex(other.capacity(), c.association(same_indices=False))
        c.census()
        self.association()
        self.census()
        return c


# ---- random operation streams ------------------------------------------------

def key_pool(rng, count):
    """`count` distinct keys of a small cube: batches drawn from it are full
    of duplicates and of keys erased earlier."""
    side = 2
    while side ** 3 < 2 * count:
        side += 1
    flat = rng.choice(side ** 3, size=count, replace=False)
    k = np.stack([flat % side, (flat // side) % side, flat // (side * side)],
                 axis=1) - side // 2
    return [_key(r) for r in k]


def _batch(rng, model, pool, inserting, max_distinct):
    """Keys with multiplicities 1..64. When inserting, the new distinct keys
    fit the free indices (the caller's side of the contract). The first key
    fills wave 0 of the launch on its own (64 consecutive occurrences)."""
    want = int(rng.integers(1, max_distinct + 1))
    order = [pool[i] for i in rng.permutation(len(pool))]
    chosen, fresh = [], 0
    for k in order:
        if len(chosen) == want:
            break
        if inserting and k not in model.entries:
            if fresh == len(model.free):
                continue
            fresh += 1
        chosen.append(k)
    if not chosen:
        chosen = [order[0]] if not inserting else \
            [k for k in order if k in model.entries][:1] or []
    if not chosen:
        return np.zeros((0, 3), np.int32)
    mult = rng.choice([1, 1, 1, 2, 3, 7, 33, 64], size=len(chosen))
    wave = rng.random() < 0.5
    body = [k for k, c in zip(chosen[1 if wave else 0:],
                              mult[1 if wave else 0:]) for _ in range(c)]
    body = [body[i] for i in rng.permutation(len(body))]
    head = [chosen[0]] * 64 if wave else []
    return np.array(head + body, np.int32).reshape(-1, 3)


def random_stream(chk, rng, n_ops, pool=None, reserve=True, max_distinct=None):
    """n_ops random batches of activate / insert / find / erase / reserve /
    clear on `chk`; size and active_indices are judged after every batch."""
    m = chk.model
    cap0 = m.capacity
    if pool is None:
        pool = key_pool(rng, 2 * cap0 + 8)
    if max_distinct is None:
        max_distinct = min(len(pool), max(4, min(cap0, 400)))
    outside = [(KEY_HI + 1, 0, 0), (0, -KEY_HI - 2, 0), (1, 2, KEY_HI + 1)]
    ops = ["activate", "insert", "insert", "find", "erase", "erase"]
    for step in range(n_ops):
        r = rng.random()
        if reserve and r < 0.12:
            size = m.size()
            kind = rng.integers(4)
            if kind == 0:                       # grow
                cap = m.capacity + int(rng.integers(1, m.capacity + 3))
            elif kind == 1 and m.capacity - size >= 2:   # shrink above size
                cap = int(rng.integers(size + 1, m.capacity))
            elif kind == 2 and size > 0:        # at or below the size: no-op
                cap = int(rng.integers(max(1, size - 2), size + 1))
            else:
                cap = cap0
            if cap != m.capacity:
                chk.reserve(cap)
            continue
        if r < 0.17:
            chk.clear()
            continue
        op = ops[int(rng.integers(len(ops)))]
        keys = _batch(rng, m, pool, op in ("activate", "insert"),
                      max_distinct)
        if op in ("find", "erase") and len(keys):
            # out-of-range keys: absent, and no error
            extra = np.array([outside[int(rng.integers(3))]], np.int32)
            at = int(rng.integers(len(keys) + 1))
            keys = np.concatenate([keys[:at], extra, keys[at:]])
        if len(keys) == 0:
            continue
        if op == "activate":
            chk.activate(keys)
        elif op == "insert":
            chk.insert(keys, distinct_rows(rng, len(keys), chk.sizes))
        elif op == "find":
            chk.find(keys)
            chk.census()
        else:
            chk.erase(keys)
    chk.association()
    for k in outside:
        assert not key_in_range(*k)
