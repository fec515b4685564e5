"""Reference model of the block hash map, and the constructions that choose
adversarial inputs for it (no GPU, no library).

Three separate things live here:

* `HashModel` / `PackedModel`: WHAT a map must answer. A Python dictionary
  key -> (buffer index, value rows) beside the set of free indices, and the same
  over packed 63-bit integers with numpy for batches of millions. The device
  chooses which occurrence of a duplicated key wins and which free index it
  gets; the model states what every choice must satisfy and then records the
  choice. Only these two judge a result.
* Restatements of KeyInRange / PackKey / HashKey (common.h) and of the table
  geometry (block_hash.hip). They serve to CHOOSE inputs (keys that share a
  home slot, chains that wrap, range limits); test_hash_model_cpu.py pins them
  to the header so that a changed hash function cannot quietly turn the
  constructions into random ones.
* `SlotSim`: a sequential restatement of the slot table (linear probing, the
  first-tombstone rule, the two 3/4 rebuild points). Its only use is to assert
  a scenario's precondition ("no empty slot is left"). It equals the device's
  table whenever every batch of one launch consists of keys whose home slots
  are distinct and directly empty (or of erases), because then no thread
  order can change which slot a key takes.
"""
import numpy as np

KEY_BIAS = 1 << 20
KEY_LO = -KEY_BIAS          # smallest valid coordinate
KEY_HI = KEY_BIAS - 1       # largest valid coordinate
_M64 = (1 << 64) - 1


# ---- restatements (input construction only) --------------------------------

def key_in_range(x, y, z):
    return all(KEY_LO <= c <= KEY_HI for c in (x, y, z))


def pack_key(x, y, z):
    return ((x + KEY_BIAS) << 42) | ((y + KEY_BIAS) << 21) | (z + KEY_BIAS)


def hash_key(k):
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & _M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & _M64
    k ^= k >> 31
    return k & 0xFFFFFFFF


def keys_in_range(keys):
    """[n,3] integer array -> bool [n]."""
    k = np.asarray(keys, np.int64)
    return ((k >= KEY_LO) & (k <= KEY_HI)).all(axis=1)


def pack_keys(keys):
    """[n,3] integer array of in-range keys -> int64 [n] (63 bits used)."""
    k = np.asarray(keys, np.int64) + KEY_BIAS
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def unpack_keys(packed):
    p = np.asarray(packed, np.int64)
    m = (1 << 21) - 1
    return np.stack([(p >> 42) & m, (p >> 21) & m, p & m],
                    axis=1).astype(np.int64) - KEY_BIAS


def hash_keys(packed):
    k = np.asarray(packed, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(30))
        k = k * np.uint64(0xbf58476d1ce4e5b9)
        k = k ^ (k >> np.uint64(27))
        k = k * np.uint64(0x94d049bb133111eb)
        k = k ^ (k >> np.uint64(31))
    return (k & np.uint64(0xFFFFFFFF)).astype(np.int64)


def n_slots(capacity):
    p = 64
    while p < 2 * capacity:
        p <<= 1
    return p


def home_slot(key, slots):
    return hash_key(pack_key(*key)) & (slots - 1)


def home_slots(keys, slots):
    return hash_keys(pack_keys(keys)) & (slots - 1)


# ---- key generators --------------------------------------------------------

_SIDE = 2001


def candidate_keys(start, count):
    """`count` distinct small keys, a fixed enumeration of [-1000,1000]^3."""
    i = np.arange(start, start + count, dtype=np.int64)
    return np.stack([i % _SIDE - 1000, (i // _SIDE) % _SIDE - 1000,
                     i // (_SIDE * _SIDE) - 1000], axis=1).astype(np.int32)


def keys_with_home(slot, slots, count, start=0, exclude=()):
    """The first `count` candidate keys (from `start` on) whose home slot in a
    table of `slots` slots is `slot`, none of them in `exclude`."""
    seen = {tuple(int(c) for c in k) for k in exclude}
    out = []
    chunk = max(4096, 64 * slots)
    while len(out) < count:
        c = candidate_keys(start, chunk)
        start += chunk
        for k in c[home_slots(c, slots) == slot]:
            t = tuple(int(v) for v in k)
            if t not in seen:
                seen.add(t)
                out.append(t)
                if len(out) == count:
                    break
        assert start < _SIDE ** 3, "candidate keys exhausted"
    return out


def one_key_per_home(homes, slots, start=0, exclude=()):
    """One key for every home slot listed, all distinct."""
    seen = [tuple(k) for k in exclude]
    out = []
    for s in homes:
        k = keys_with_home(int(s), slots, 1, start, seen)[0]
        seen.append(k)
        out.append(k)
    return out


def wrapping_chain(slots, length, tail=3, start=0):
    """`length` keys sharing the home slot `slots - tail`: inserted one after
    the other, their chain runs over the last slot and on from slot 0."""
    assert length > tail
    return keys_with_home(slots - tail, slots, length, start)


def range_limit_keys():
    """(valid, invalid): valid keys with every coordinate drawn from the
    values at and next to both limits (and -1, 0), so that each limit meets
    the other two coordinates at their extremes and a packing fault aliases
    two of them; invalid keys with at least one coordinate one step outside,
    again beside extremes."""
    v = (KEY_LO, KEY_LO + 1, -1, 0, KEY_HI - 1, KEY_HI)
    valid = [(x, y, z) for x in v for y in v for z in v]
    w = (KEY_LO - 1, KEY_LO, 0, KEY_HI, KEY_HI + 1)
    invalid = [(x, y, z) for x in w for y in w for z in w
               if not key_in_range(x, y, z)]
    return valid, invalid


# ---- the dictionary model --------------------------------------------------

class HashModel:
    """key tuple -> [buffer index, [value row bytes per value array]]."""

    def __init__(self, capacity, value_sizes=()):
        self.capacity = int(capacity)
        self.value_sizes = tuple(int(s) for s in value_sizes)
        self.entries = {}
        self.free = set(range(self.capacity))
        self.pristine = True    # fresh or cleared: indices come out as 0..m-1

    # -- expectations (pure) --
    @staticmethod
    def _occurrences(keys):
        occ = {}
        for i, k in enumerate(keys):
            occ.setdefault(tuple(int(c) for c in k), []).append(i)
        return occ

    def new_keys(self, keys):
        """{key: [positions]} of the in-range keys of a batch that are absent
        now: each must get exactly one winner."""
        return {k: p for k, p in self._occurrences(keys).items()
                if key_in_range(*k) and k not in self.entries}

    def present_keys(self, keys):
        """{key: [positions]} of the batch keys that are present now."""
        return {k: p for k, p in self._occurrences(keys).items()
                if k in self.entries}

    def find(self, keys):
        """(masks, indices) a Find of `keys` must return."""
        m = np.zeros(len(keys), bool)
        idx = np.zeros(len(keys), np.int64)
        for i, k in enumerate(keys):
            e = self.entries.get(tuple(int(c) for c in k))
            if e is not None:
                m[i], idx[i] = True, e[0]
        return m, idx

    def size(self):
        return len(self.entries)

    def active(self):
        return {e[0] for e in self.entries.values()}

    # -- recording what the device chose (checked against the free set) --
    def commit_insert(self, key, idx, rows=None):
        key = tuple(int(c) for c in key)
        assert key not in self.entries and key_in_range(*key)
        assert idx in self.free, "index %d is not free" % idx
        self.free.remove(idx)
        if rows is None:
            rows = [bytes(s) for s in self.value_sizes]   # zero filled
        self.entries[key] = [int(idx), [bytes(r) for r in rows]]

    def commit_erase(self, key):
        idx = self.entries.pop(tuple(int(c) for c in key))[0]
        self.free.add(idx)
        self.pristine = False

    def clear(self):
        self.entries = {}
        self.free = set(range(self.capacity))
        self.pristine = True

    def reindex(self, capacity, new_index):
        """After Reserve / To: a map of `capacity` entries, every key at
        new_index[key]; rows stay attached to their keys."""
        assert set(new_index) == set(self.entries)
        idx = [int(i) for i in new_index.values()]
        assert len(set(idx)) == len(idx)
        assert all(0 <= i < capacity for i in idx)
        self.capacity = int(capacity)
        for k, i in new_index.items():
            self.entries[k][0] = int(i)
        self.free = set(range(self.capacity)) - set(idx)
        self.pristine = False

    def copy(self):
        m = HashModel(self.capacity, self.value_sizes)
        m.entries = {k: [e[0], list(e[1])] for k, e in self.entries.items()}
        m.free = set(self.free)
        m.pristine = self.pristine
        return m


# ---- the same over packed keys, vectorised ----------------------------------

class PackedModel:
    """Sorted int64 packed keys beside their buffer indices (hash set: no
    value rows). Judges batches of millions with np.unique / np.isin."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.keys = np.zeros(0, np.int64)
        self.idx = np.zeros(0, np.int64)
        self.pristine = True

    def size(self):
        return len(self.keys)

    def lookup(self, packed):
        """(present, index) per packed key; index 0 where absent."""
        pos = np.searchsorted(self.keys, packed)
        pos = np.minimum(pos, max(len(self.keys) - 1, 0))
        hit = (self.keys[pos] == packed) if len(self.keys) else \
            np.zeros(len(packed), bool)
        return hit, np.where(hit, self.idx[pos] if len(self.keys) else 0, 0)

    def check_insert(self, keys, masks, idx, key_buffer):
        """Judges one activate launch and records its winners."""
        keys = np.asarray(keys)
        masks = np.asarray(masks, bool)
        idx = np.asarray(idx, np.int64)
        ok = keys_in_range(keys)
        assert not masks[~ok].any() and not idx[~ok].any()
        packed = pack_keys(keys[ok])
        mk, ix = masks[ok], idx[ok]
        uniq, inv = np.unique(packed, return_inverse=True)
        present, _ = self.lookup(uniq)
        wins = np.bincount(inv, weights=mk, minlength=len(uniq)).astype(int)
        assert np.array_equal(wins, (~present).astype(int)), \
            "every new key needs exactly one winner, a present key none"
        assert not ix[~mk].any(), "losers must report index 0"
        widx = ix[mk]
        assert len(np.unique(widx)) == len(widx), "winners share an index"
        assert widx.min(initial=0) >= 0 and \
            widx.max(initial=0) < self.capacity
        assert not np.isin(widx, self.idx).any(), "a live index handed out"
        if self.pristine and len(self.keys) == 0:
            assert np.array_equal(np.sort(widx), np.arange(len(widx))), \
                "a fresh map hands out 0..m-1"
        assert np.array_equal(np.asarray(key_buffer)[widx], keys[ok][mk])
        k = np.concatenate([self.keys, packed[mk]])
        i = np.concatenate([self.idx, widx])
        o = np.argsort(k, kind="stable")
        self.keys, self.idx = k[o], i[o]
        assert len(np.unique(self.keys)) == len(self.keys)

    def check_find(self, keys, masks, idx):
        keys = np.asarray(keys)
        ok = keys_in_range(keys)
        want_m = np.zeros(len(keys), bool)
        want_i = np.zeros(len(keys), np.int64)
        want_m[ok], want_i[ok] = self.lookup(pack_keys(keys[ok]))
        assert np.array_equal(np.asarray(masks, bool), want_m)
        assert np.array_equal(np.asarray(idx, np.int64), want_i)

    def check_erase(self, keys, masks):
        keys = np.asarray(keys)
        masks = np.asarray(masks, bool)
        ok = keys_in_range(keys)
        assert not masks[~ok].any()
        packed = pack_keys(keys[ok])
        uniq, inv = np.unique(packed, return_inverse=True)
        present, _ = self.lookup(uniq)
        wins = np.bincount(inv, weights=masks[ok],
                           minlength=len(uniq)).astype(int)
        assert np.array_equal(wins, present.astype(int)), \
            "every present key is erased by exactly one occurrence"
        keep = ~np.isin(self.keys, uniq[present])
        self.keys, self.idx = self.keys[keep], self.idx[keep]
        self.pristine = False

    def check_active(self, count, indices):
        assert count == len(self.keys)
        assert np.array_equal(np.sort(np.asarray(indices, np.int64)[:count]),
                              np.sort(self.idx))

    def clear(self):
        self.keys = np.zeros(0, np.int64)
        self.idx = np.zeros(0, np.int64)
        self.pristine = True


# ---- sequential simulator of the slot table ---------------------------------

class SlotSim:
    """What block_hash.hip's table looks like after launches whose outcome no
    thread order can change. EMPTY / TOMB / key tuple per slot; `taken` is the
    device's count of slots ever taken from the empty state since the last
    rebuild (live + tombstones)."""
    EMPTY = None
    TOMB = "tomb"

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.n = n_slots(capacity)
        self.slots = [self.EMPTY] * self.n
        self.taken = 0
        self.rebuilds = 0

    def home(self, key):
        return home_slot(key, self.n)

    def insert(self, key):
        """Insert-if-absent; the slot the key lives in, and whether new."""
        key = tuple(int(c) for c in key)
        h = self.home(key)
        tomb = None
        for _ in range(self.n):
            cur = self.slots[h]
            if cur == key:
                return h, False
            if cur is self.TOMB:
                if tomb is None:
                    tomb = h
            elif cur is self.EMPTY:
                if tomb is None:
                    self.taken += 1
                    tomb = h
                self.slots[tomb] = key
                return tomb, True
            h = (h + 1) % self.n
        # a whole cycle without an empty slot: the first tombstone
        assert tomb is not None, "table full of live keys"
        self.slots[tomb] = key
        return tomb, True

    def find(self, key):
        key = tuple(int(c) for c in key)
        h = self.home(key)
        for _ in range(self.n):
            cur = self.slots[h]
            if cur == key:
                return h
            if cur is self.EMPTY:
                return None
            h = (h + 1) % self.n
        return None

    def crowded(self):
        return self.taken * 4 >= self.n * 3

    def _maybe_rebuild(self):
        if not self.crowded():
            return False
        live = self.live()
        self.slots = [self.EMPTY] * self.n
        self.taken = 0
        for k in live:      # order only matters among colliding keys
            self.insert(k)
        self.rebuilds += 1
        return True

    def erase_batch(self, keys):
        """One Erase launch: tombstones, then the rebuild check behind it."""
        for key in keys:
            s = self.find(key)
            if s is not None:
                self.slots[s] = self.TOMB
        return self._maybe_rebuild()

    def size_call(self):
        """o3dmi_hash_size (and everything that goes through it)."""
        return self._maybe_rebuild()

    def live(self):
        return [s for s in self.slots
                if s is not self.EMPTY and s is not self.TOMB]

    def empty_slots(self):
        return [i for i, s in enumerate(self.slots) if s is self.EMPTY]

    def tombstones(self):
        return [i for i, s in enumerate(self.slots) if s is self.TOMB]


def crowding_plan(capacity=64, start=0, spare=8):
    """The batches that lead a `capacity`-entry map to a table with no empty
    slot by inserts alone, as a list of ("insert" | "erase", [keys]).

    Every insert batch consists of keys whose home slots are distinct and
    empty at that moment, so each key sits in its home slot whatever the
    thread order. With n = n_slots(capacity) and the rebuild mark at
    taken >= 3n/4: after the last erase `taken` must be 3n/4 - 1, and the
    n - taken remaining empty slots must fit beside the live keys, so the
    live count after that erase is at most capacity - (n/4 + 1); `spare`
    more indices are left free for what a test inserts into the full table.

    Returns (plan, index of the batch whose inserts cross the 3/4 mark)."""
    n = n_slots(capacity)
    assert n == 2 * capacity and capacity % 4 == 0 and capacity >= 16
    mark = 3 * n // 4
    sim = SlotSim(capacity)
    plan, used = [], []

    def insert_into_empty(count):
        keys = one_key_per_home(sim.empty_slots()[:count], n, start, used)
        for k in keys:
            slot, new = sim.insert(k)
            assert new and slot == sim.home(k)
        used.extend(keys)
        plan.append(("insert", keys))
        return keys

    def erase(keys):
        assert not sim.erase_batch(keys), "this erase must not rebuild"
        plan.append(("erase", list(keys)))

    first = insert_into_empty(capacity)                 # taken = n/2
    keep = capacity - (n // 4 + 1) - spare              # live after 2nd erase
    erase(first[keep:])
    second = insert_into_empty(mark - 1 - sim.taken)    # taken = mark - 1
    assert len(sim.live()) <= capacity
    erase(second)
    assert sim.taken == mark - 1 and not sim.crowded()
    assert len(sim.live()) == keep
    crossing = len(plan)
    insert_into_empty(n - sim.taken)                    # every empty slot
    assert sim.taken == n and not sim.empty_slots()
    assert len(sim.live()) == capacity - spare
    return plan, crossing


def replay(plan, capacity, upto=None):
    """The simulator after the first `upto` batches of a plan."""
    sim = SlotSim(capacity)
    for op, keys in plan[:upto]:
        if op == "insert":
            for k in keys:
                sim.insert(k)
        else:
            sim.erase_batch(keys)
    return sim
