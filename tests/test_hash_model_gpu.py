"""The block hash map (block_hash.hip, ClaimSlot / HashView::Find in common.h,
the row gather / scatter of rows.hip) against a dictionary model, through the
C ABI. Every batch is one launch and every batch is judged (_hash_check.py);
the scenario preconditions come from the host simulator (_hash_model.py),
never from the device, whose slot table the ABI does not expose.

Ownership settings of o3dmi_hash_to_device are not checked here: observing
them takes a depth-touch launch with a camera and an image, which is not cheap
beside these tests; tests/test_sharding.py covers the sharded grids.

Measured run time of this file on one MI355X: 8 s for its 37 tests (the two
large cases take 1.9 s and 1.4 s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _hash_check as hc
import _hash_model as hm

pytestmark = pytest.mark.gpu

OK, ERR_CAPACITY, ERR_KEY_RANGE = 0, 3, 4


class DeviceMap:
    """One o3dmi_hash_t behind the driver interface of _hash_check.Checker."""

    def __init__(self, capacity=None, sizes=(), handle=None):
        if not torch.cuda.is_available():
            pytest.skip("needs a GPU")
        from open3d_amd import _lib
        from open3d_amd.core import stream, tensor_from_ptr
        self._lib, self.L = _lib, _lib.lib()
        self._stream, self._view = stream, tensor_from_ptr
        self.sizes = tuple(int(s) for s in sizes)
        self.h = handle
        if handle is None:
            self.h = C.c_void_p()
            ds = (C.c_int64 * max(1, len(self.sizes)))(*self.sizes)
            _lib.check(self.L.o3dmi_hash_create(
                capacity, len(self.sizes), ds, stream(), C.byref(self.h)),
                "create")

    def destroy(self):
        if self.h:
            torch.cuda.synchronize()
            self.L.o3dmi_hash_destroy(self.h)
            self.h = None

    def capacity(self):
        return int(self.L.o3dmi_hash_capacity(self.h))

    def slots(self):
        return int(self.L.o3dmi_hash_bucket_count(self.h))

    def _out(self, n):
        return (torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                torch.full((n,), 9, dtype=torch.uint8, device="cuda"))

    @staticmethod
    def _masks(m):
        m = m.cpu().numpy()
        assert ((m == 0) | (m == 1)).all(), "a mask is neither 0 nor 1"
        return m.astype(bool)

    def activate(self, keys):
        k = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).cuda()
        b, m = self._out(len(keys))
        p = self._lib.ptr
        self._lib.check(self.L.o3dmi_hash_activate(
            self.h, p(k), len(keys), None, p(b), p(m), self._stream()),
            "activate")
        return b.cpu().numpy(), self._masks(m)

    def insert(self, keys, rows):
        if not self.sizes:
            rows = []
        assert len(rows) == len(self.sizes)
        k = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).cuda()
        v = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rows]
        for t, s in zip(v, self.sizes):
            assert t.shape == (len(keys), s) and t.dtype == torch.uint8
        vp = (C.c_void_p * len(v))(*[t.data_ptr() for t in v]) if v else None
        b, m = self._out(len(keys))
        p = self._lib.ptr
        self._lib.check(self.L.o3dmi_hash_insert(
            self.h, p(k), vp, len(keys), p(b), p(m), self._stream()),
            "insert")
        return b.cpu().numpy(), self._masks(m)

    def find(self, keys):
        k = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).cuda()
        b, m = self._out(len(keys))
        p = self._lib.ptr
        self._lib.check(self.L.o3dmi_hash_find(
            self.h, p(k), len(keys), None, p(b), p(m), self._stream()),
            "find")
        return b.cpu().numpy(), self._masks(m)

    def erase(self, keys):
        k = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).cuda()
        _, m = self._out(len(keys))
        p = self._lib.ptr
        self._lib.check(self.L.o3dmi_hash_erase(
            self.h, p(k), len(keys), p(m), self._stream()), "erase")
        return self._masks(m)

    def size(self):
        n = C.c_int64(-1)
        st = self.L.o3dmi_hash_size(self.h, self._stream(), C.byref(n))
        return st, n.value

    def active(self):
        # one entry per SLOT, not per index: a count beyond the capacity
        # would then be a failed assertion, not a write out of bounds
        out = torch.full((self.slots(),), -5, dtype=torch.int32,
                         device="cuda")
        n = C.c_int64(-1)
        self._lib.check(self.L.o3dmi_hash_active_indices(
            self.h, self._lib.ptr(out), self._stream(), C.byref(n)), "active")
        assert 0 <= n.value <= self.capacity(), n.value
        return out[:n.value].cpu().numpy()

    def reserve(self, capacity):
        return self.L.o3dmi_hash_reserve(self.h, capacity, self._stream())

    def clear(self):
        self._lib.check(self.L.o3dmi_hash_clear(self.h, self._stream()),
                        "clear")

    def key_buffer(self):
        return self._view(self.L.o3dmi_hash_key_buffer(self.h),
                          (self.capacity(), 3), self._lib.I32,
                          None).cpu().numpy()

    def value_buffer(self, j):
        return self._view(self.L.o3dmi_hash_value_buffer(self.h, j),
                          (self.capacity(), self.sizes[j]), self._lib.U8,
                          None).cpu().numpy()

    def to_device(self):
        torch.cuda.synchronize()
        out = C.c_void_p()
        self._lib.check(self.L.o3dmi_hash_to_device(
            self.h, torch.cuda.current_device(), C.byref(out)), "to_device")
        return DeviceMap(sizes=self.sizes, handle=out)


@pytest.fixture
def maps():
    made = []

    def make(capacity, sizes=()):
        d = DeviceMap(capacity, sizes)
        made.append(d)
        return d

    make.adopt = made.append
    yield make
    for d in made:
        d.destroy()


# ---- 1. random operation streams ---------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("capacity", [1, 2, 63, 64, 65, 3000])
def test_random_streams(maps, capacity, seed):
    """activate / insert / find / erase / size / active_indices / reserve
    (growing, shrinking above the size, no-op at or below it) / clear, from a
    key pool small enough that batches are full of duplicates (1 to 64 of a
    key, a whole wave of one key included) and of keys erased earlier."""
    rng = np.random.default_rng(1000 * capacity + seed)
    sizes = (4, 3)
    chk = hc.Checker(maps(capacity, sizes), sizes)
    hc.random_stream(chk, rng, 30 if capacity >= 1000 else 60)


# ---- 2. duplicates behind tombstones -------------------------------------------

@pytest.mark.parametrize("wrap", [False, True])
def test_duplicates_behind_tombstones(maps, wrap):
    """ClaimSlot's central claim: every inserter of one key competes for the
    same slot -- the first tombstone of the probe sequence, but only after the
    walk has gone on to the empty slot, because the key may live behind the
    tombstone. One launch holds duplicates of new keys of a chain with a
    stripe of tombstones, other new keys that collide with them, and keys
    still present behind the tombstones."""
    cap, sizes = 64, (4,)
    slots = hm.n_slots(cap)
    rng = np.random.default_rng(21 + wrap)
    home = slots - 3 if wrap else 20
    chain = hm.wrapping_chain(slots, 12) if wrap else \
        hm.keys_with_home(home, slots, 12)
    sim = hm.SlotSim(cap)
    chk = hc.Checker(maps(cap, sizes), sizes)
    for k in chain:         # one launch each: the chain order is the sim's
        chk.insert([k], hc.distinct_rows(rng, 1, sizes))
        sim.insert(k)
    at = [sim.find(k) for k in chain]
    assert at == [(home + i) % slots for i in range(12)]
    assert (min(at) == 0 and max(at) == slots - 1) == wrap
    stripe = chain[1::2][:5]                  # chain[11] stays, behind them
    chk.erase(stripe)
    assert not sim.erase_batch(stripe)
    assert sim.tombstones() == sorted(at[i] for i in (1, 3, 5, 7, 9))
    behind = chain[2::2] + [chain[11]]        # live, tombstones before them
    fresh = hm.keys_with_home(home, slots, 3, exclude=chain)
    colliders = hm.one_key_per_home(
        [(home + 2) % slots, (home + 5) % slots, (home + 13) % slots], slots,
        exclude=chain + fresh)
    batch = [k for k in fresh for _ in range(20)] + \
        [k for k in colliders for _ in range(5)] + \
        [k for k in behind for _ in range(3)] + [stripe[0]] * 4
    batch = [batch[i] for i in rng.permutation(len(batch))]
    chk.insert(batch, hc.distinct_rows(rng, len(batch), sizes))
    chk.association()
    everything = list(chk.model.entries)
    assert len(everything) == 12 - 5 + 3 + 3 + 1
    chk.find(everything + stripe[1:])
    dup = [k for k in everything for _ in range(3)] + stripe[1:]
    chk.erase([dup[i] for i in rng.permutation(len(dup))])
    assert chk.model.size() == 0


# ---- 3. / 4. crowded tables ----------------------------------------------------

def _run_plan(chk, rng, plan):
    for op, keys in plan:
        if op == "insert":
            chk.insert(keys, hc.distinct_rows(rng, len(keys), chk.sizes))
        else:
            chk.erase(keys)


def _absent_keys(chk, rng, n):
    out = []
    while len(out) < n:
        k = tuple(int(c) for c in rng.integers(2000, 9000, size=3))
        if k not in chk.model.entries and k not in out:
            out.append(k)
    return out


@pytest.mark.timeout(300)
def test_table_without_an_empty_slot(maps):
    """128 slots, all of them live keys or tombstones, reached by inserts
    into empty home slots with no Erase and no Size after the 3/4 mark. Find
    of an absent key ends by its bound; a new key, inserted twice in one
    launch, takes a tombstone through ClaimSlot's whole-cycle branch; the
    next Size rebuilds and moves no key. Then six new keys of one home slot in
    one launch: in a rebuilt table their walks end at once, in a table still
    full each lost CAS costs a whole cycle and ClaimSlot's step bound sets the
    probe-wrap error."""
    cap, sizes = 64, (4, 6)
    rng = np.random.default_rng(33)
    plan, crossing = hm.crowding_plan(cap)
    sim = hm.replay(plan, cap)
    assert sim.empty_slots() == [] and sim.rebuilds == 0      # precondition
    chk = hc.Checker(maps(cap, sizes), sizes)
    _run_plan(chk, rng, plan[:crossing])
    keys = plan[crossing][1]
    chk.insert(keys, hc.distinct_rows(rng, len(keys), sizes), size=False)
    assert chk.model.size() == len(sim.live()) == cap - 8
    absent = _absent_keys(chk, rng, 64)
    chk.find(absent + [(hm.KEY_HI + 1, 0, 0)])
    chk.association()                       # live keys found, no empty slot
    new = absent[0]
    chk.insert([new, new], hc.distinct_rows(rng, 2, sizes), size=False)
    chk.find(absent)
    chk.census(size=True)                   # Size: the rebuild
    chk.association()                       # same indices, same rows
    chk.find(absent[1:])
    same_home = hm.keys_with_home(sim.home(absent[1]), sim.n, 6,
                                  exclude=list(chk.model.entries))
    chk.insert(same_home, hc.distinct_rows(rng, 6, sizes))
    chk.association()
    hc.random_stream(chk, rng, 20, reserve=False,
                     pool=list(chk.model.entries) + hc.key_pool(rng, 80))


@pytest.mark.timeout(300)
def test_crowded_by_inserts_not_by_erase(maps):
    """live + tombstones pass 3/4 of the slots on an insert, with the last
    Erase one below the mark: the rebuild must come from the next Size."""
    cap, sizes = 64, (4, 6)
    rng = np.random.default_rng(44)
    plan, crossing = hm.crowding_plan(cap)
    sim = hm.replay(plan, cap, crossing)
    assert sim.taken == 3 * sim.n // 4 - 1 and sim.rebuilds == 0
    some = plan[crossing][1][:5]
    for k in some:
        sim.insert(k)
    assert sim.crowded() and sim.empty_slots()                # precondition
    chk = hc.Checker(maps(cap, sizes), sizes)
    _run_plan(chk, rng, plan[:crossing])
    chk.insert(some, hc.distinct_rows(rng, 5, sizes), size=False)
    chk.census(size=True)                   # Size: the rebuild
    chk.association()
    chk.find(_absent_keys(chk, rng, 64))
    hc.random_stream(chk, rng, 40,
                     pool=list(chk.model.entries) + hc.key_pool(rng, 80))


# ---- 5. beyond one launch grid -------------------------------------------------

def _big_map_calls(dev, pm):
    def activate(keys):
        idx, mask = dev.activate(keys)
        pm.check_insert(keys, mask, idx, dev.key_buffer())

    def find(keys):
        idx, mask = dev.find(keys)
        pm.check_find(keys, mask, idx)

    def erase(keys):
        pm.check_erase(keys, dev.erase(keys))

    def census():
        act = dev.active()
        pm.check_active(len(act), act)
        assert dev.size() == (OK, pm.size())

    return activate, find, erase, census


@pytest.mark.timeout(900)
def test_beyond_one_launch_grid(maps):
    """More keys than the 2048 x 256 threads of one launch (Activate, Find,
    Erase) and 2^22 slots for ActiveIndicesKernel's ballot stride."""
    cap = 2 << 20
    rng = np.random.default_rng(55)
    dev = maps(cap)
    assert dev.slots() == 1 << 22
    pm = hm.PackedModel(cap)
    activate, find, erase, census = _big_map_calls(dev, pm)
    pool = hm.candidate_keys(0, 3_000_000)
    pool = pool[rng.permutation(len(pool))]
    first, later, never = pool[:1_000_000], pool[1_000_000:1_400_000], \
        pool[1_400_000:]
    n = 1_500_001
    assert n > 2048 * 256 and n % 64
    batch = np.concatenate([first, first[rng.integers(0, len(first),
                                                      n - len(first))]])
    batch = batch[rng.permutation(n)]
    activate(batch)
    assert pm.size() == 1_000_000
    census()
    probe = np.concatenate([first[:750_000], never[:750_001]])
    probe[5] = (hm.KEY_HI + 1, 0, 0)
    find(probe[rng.permutation(len(probe))])
    gone = first[rng.integers(0, 400_000, 550_001)]     # duplicates
    gone = np.concatenate([gone, never[:50_000]])       # and absent keys
    erase(gone[rng.permutation(len(gone))])
    assert 250_000 < pm.size() < 1_000_000 - 250_000
    census()
    find(first)
    again = np.concatenate([first[:400_000], later, later[:100_001]])
    activate(again[rng.permutation(len(again))])
    census()
    find(pool[:1_500_001])


# ---- 6. clear beyond its capped grid -------------------------------------------

@pytest.mark.timeout(900)
def test_clear_beyond_its_capped_grid(maps):
    """ClearKernel's launch is capped at 4096 groups x 256 threads x 8 slots
    = 2^23 slots; a map of 2^24 slots needs its second stride.

    Device memory of this map (AllocateStorage): per slot 8 (key) + 4 (index)
    + 16 (two touch planes) bytes, per entry 4 (heap) + 12 (key buffer):
    2^24 * 28 + (2^22 + 1) * 16 = 536 870 928 bytes, 512 MiB."""
    cap = (1 << 22) + 1
    slots = hm.n_slots(cap)
    need = slots * 28 + cap * 16
    assert slots == 1 << 24 and need == 536_870_928
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib
    mem = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_device_info(None, 0, None, C.byref(mem)),
               "device_info")
    if mem.value < 4 * need:
        pytest.skip("the device has %d bytes, this case wants 4 x %d"
                    % (mem.value, need))
    rng = np.random.default_rng(66)
    dev = maps(cap)
    assert dev.slots() == slots
    pm = hm.PackedModel(cap)
    activate, find, erase, census = _big_map_calls(dev, pm)
    cand = hm.candidate_keys(0, 1 << 23)
    home = hm.home_slots(cand, slots)
    last = cand[home >= slots - 4096]           # the last slots' keys
    assert len(last) > 500 and (home >= slots - 64).any()
    spread = cand[rng.permutation(len(cand))[:1 << 20]]
    keys = np.unique(np.concatenate([last, spread]), axis=0)
    hk = hm.home_slots(keys, slots)
    # every 64th part of the table is hit, both strides of Clear included
    assert len(np.unique(hk >> 18)) == 64
    activate(keys[rng.permutation(len(keys))])
    census()
    dev.clear()
    pm.clear()
    census()                                    # size 0, no active index
    find(np.concatenate([last, spread]))        # all absent again
    m = 100_003
    activate(cand[(1 << 22):(1 << 22) + m])     # check_insert: {0..m-1}
    assert pm.pristine and set(pm.idx.tolist()) == set(range(m))
    census()


# ---- 7. value layouts ----------------------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("sizes", [
    (),                                  # a hash set
    (1,), (16384,),                      # byte form / one block-sized row
    (2, 12, 48), (6, 4, 16),             # byte, word and 16-byte forms
    (1, 2, 6, 4, 12, 20, 16, 48),        # 8 arrays, every form
], ids=lambda s: "x".join(map(str, s)) or "set")
def test_value_layouts(maps, sizes):
    """Rows of 1, 2, 6 bytes take RowsKernel's byte form in Reserve and To,
    4, 12, 20 the word form, 16, 48, 16384 the 16-byte form; Insert copies
    them byte by byte for up to 8 arrays."""
    cap = 40 if 16384 in sizes else 300
    rng = np.random.default_rng(len(sizes) * 7 + sum(sizes))
    chk = hc.Checker(maps(cap, sizes), sizes)
    pool = hc.key_pool(rng, cap)
    keys = [pool[i] for i in rng.integers(0, cap // 2, 3 * cap)]
    chk.insert(keys, hc.distinct_rows(rng, len(keys), sizes))
    chk.reserve(2 * cap + 1)                            # grow
    chk.erase(keys[:cap // 4])
    chk.reserve(chk.model.size() + 3)                   # shrink
    chk.reserve(max(1, chk.model.size() - 1))           # no-op
    more = [pool[cap // 2 + i % 3] for i in range(9)]
    chk.insert(more, hc.distinct_rows(rng, 9, sizes))
    assert chk.model.size() == chk.model.capacity       # no slack left
    other = chk.to_device()                 # same capacity and association,
    maps.adopt(other.dev)                   # source unchanged (checked there)
    # independent afterwards: erase in one, find in the other, both ways
    k = list(chk.model.entries)
    other.erase(k[:5])
    chk.find(k)
    chk.association()
    chk.erase(k[5:9])
    other.find(k)
    other.association()
    chk.reserve(cap)
    hc.random_stream(chk, rng, 15, pool=pool)
    hc.random_stream(other, rng, 15, pool=pool)


# ---- 8. key range --------------------------------------------------------------

def test_key_range_limits(maps):
    """-2^20 and 2^20 - 1 are valid in every coordinate, beside any extremes
    of the other two; each such key is a key of its own. One step outside is
    absent for Find and Erase without an error; in an Activate batch it sets
    O3DMI_ERR_KEY_RANGE and leaves the batch's other keys inserted."""
    valid, invalid = hm.range_limit_keys()
    sizes = (12,)
    rng = np.random.default_rng(88)
    chk = hc.Checker(maps(len(valid) + 8, sizes), sizes)
    batch = valid + valid[::3]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    chk.insert(batch, hc.distinct_rows(rng, len(batch), sizes))
    assert chk.model.size() == len(valid)
    chk.find(valid + invalid)
    chk.association()
    chk.erase(valid[::2] + invalid + valid[::4])
    chk.find(valid + invalid)
    assert chk.dev.size() == (OK, len(valid) - len(valid[::2]))
    chk.activate(valid)
    # one key outside among new ones
    fresh = [(5, 5, 5), (hm.KEY_LO, 6, hm.KEY_HI), (-7, -7, -7)]
    mixed = fresh[:2] + [(0, hm.KEY_HI + 1, 0)] + fresh[2:]
    chk.activate(mixed, size=False)
    chk.find(mixed)
    assert chk.dev.size()[0] == ERR_KEY_RANGE
    chk.clear()                             # the flags go with the contents
    chk.insert(valid, hc.distinct_rows(rng, len(valid), sizes))


# ---- 9. capacity overflow on the direct path -----------------------------------

@pytest.mark.parametrize("with_values", [False, True])
@pytest.mark.parametrize("capacity,extra", [(50, 13), (1, 3), (64, 64)])
def test_capacity_overflow_direct_path(maps, capacity, extra, with_values):
    """capacity + k distinct keys in one launch: an error status, `capacity`
    winners with the indices 0..capacity-1, and every key without an index
    ABSENT afterwards (its slot carries the marker -1), for Find and for
    GetActiveIndices. No index of a losing key is used anywhere. Clear makes
    the map usable again."""
    sizes = (4, 3)
    rng = np.random.default_rng(capacity + extra)
    dev = maps(capacity, sizes)
    keys = np.array(hc.key_pool(rng, capacity + extra), np.int32)
    if with_values:
        rows = hc.distinct_rows(rng, len(keys), sizes)
        idx, mask = dev.insert(keys, rows)
    else:
        idx, mask = dev.activate(keys)
    assert mask.sum() == capacity
    assert sorted(idx[mask].tolist()) == list(range(capacity))
    assert not idx[~mask].any()
    st, _ = dev.size()
    assert st == ERR_CAPACITY
    fidx, fmask = dev.find(keys)
    assert np.array_equal(fmask, mask), "a key without an index is found"
    assert np.array_equal(fidx, idx)
    assert sorted(dev.active().tolist()) == list(range(capacity))
    kb = dev.key_buffer()
    assert np.array_equal(kb[idx[mask]], keys[mask])
    if with_values:
        for j in range(len(sizes)):
            assert np.array_equal(dev.value_buffer(j)[idx[mask]],
                                  rows[j][mask])
    dev.clear()
    chk = hc.Checker(dev, sizes)
    chk.census()
    chk.find(keys)
    hc.random_stream(chk, rng, 25)
