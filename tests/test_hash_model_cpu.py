"""The hash-map model, its input constructions and the shared checker, tested
without a GPU.

* The restated KeyInRange / PackKey / HashKey are pinned to
  open3d_amd/csrc/common.h by a small host program compiled with the build's
  hipcc (the functions are __host__ __device__).
* The model, the slot simulator and the scenario constructions are tested on
  their own.
* The checker runs on a plain-Python map, once right and once with each of a
  few faults, and must reject every faulty one.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _hash_check as hc
import _hash_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PIN_SRC = r"""
#include <cstdio>
#include <vector>
#include "common.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int k[3];
    while (fread(k, sizeof(int), 3, in) == 3) {
        unsigned long long r[3];
        r[0] = o3dmi::KeyInRange(k[0], k[1], k[2]) ? 1 : 0;
        r[1] = r[0] ? o3dmi::PackKey(k[0], k[1], k[2]) : 0;
        r[2] = r[0] ? o3dmi::HashKey(r[1]) : 0;
        fwrite(r, sizeof(unsigned long long), 3, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
"""


def test_restated_key_functions_match_common_h(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc here: the pin needs the build's compiler")
    src = tmp_path / "pin.cpp"
    src.write_text(_PIN_SRC)
    exe = tmp_path / "pin"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1",
                    "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "open3d_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    rng = np.random.default_rng(11)
    valid, invalid = hm.range_limit_keys()
    lim = 1 << 20
    keys = np.concatenate([
        np.array(valid + invalid, np.int64),
        rng.integers(-lim, lim, size=(12000, 3)),
        rng.integers(-40, 40, size=(4000, 3)),
        rng.integers(-lim - 3, lim + 3, size=(2000, 3)),
        rng.integers(-2 ** 31, 2 ** 31, size=(500, 3)),
        hm.candidate_keys(0, 2000).astype(np.int64)]).astype(np.int32)
    (tmp_path / "in.bin").write_bytes(keys.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"),
                    str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", np.uint64).reshape(-1, 3)
    assert len(got) == len(keys) >= 10000 + len(valid) + len(invalid)
    ok = hm.keys_in_range(keys)
    assert np.array_equal(got[:, 0].astype(bool), ok)
    assert ok[:len(valid)].all() and not ok[len(valid):][:len(invalid)].any()
    packed = hm.pack_keys(keys[ok])
    assert np.array_equal(got[ok, 1].astype(np.int64), packed)
    assert np.array_equal(got[ok, 2].astype(np.int64), hm.hash_keys(packed))
    # the scalar forms are the ones the simulator uses
    for k, g in list(zip(keys, got))[:len(valid) + len(invalid) + 2000]:
        k = tuple(int(c) for c in k)
        assert hm.key_in_range(*k) == bool(g[0])
        if g[0]:
            assert hm.pack_key(*k) == int(g[1])
            assert hm.hash_key(hm.pack_key(*k)) == int(g[2])
    assert np.array_equal(hm.unpack_keys(packed), keys[ok])


def test_table_geometry():
    assert [hm.n_slots(c) for c in (1, 2, 31, 32, 33, 63, 64, 65, 3000)] == \
        [64, 64, 64, 64, 128, 128, 128, 256, 8192]
    assert hm.n_slots(2 << 20) == 1 << 22
    assert hm.n_slots((1 << 22) + 1) == 1 << 24


def test_range_limit_keys_are_distinct_and_split_by_validity():
    valid, invalid = hm.range_limit_keys()
    assert len(set(valid)) == len(valid) and len(set(invalid)) == len(invalid)
    assert all(hm.key_in_range(*k) for k in valid)
    assert not any(hm.key_in_range(*k) for k in invalid)
    for c in range(3):
        for v in (hm.KEY_LO, hm.KEY_HI):
            others = {tuple(k[i] for i in range(3) if i != c)
                      for k in valid if k[c] == v}
            # the limit meets both other coordinates at all four extremes
            assert {(a, b) for a in (hm.KEY_LO, hm.KEY_HI)
                    for b in (hm.KEY_LO, hm.KEY_HI)} <= others
        for v in (hm.KEY_LO - 1, hm.KEY_HI + 1):
            assert any(k[c] == v and all(
                k[i] in (hm.KEY_LO, hm.KEY_HI) for i in range(3) if i != c)
                for k in invalid)
    assert len(set(hm.pack_keys(np.array(valid)).tolist())) == len(valid)
    # y packed one bit short would alias two of them
    bad = {((x + hm.KEY_BIAS) << 42) | ((y + hm.KEY_BIAS) << 20) |
           (z + hm.KEY_BIAS) for x, y, z in valid}
    assert len(bad) < len(valid)


def test_generators_hit_their_home_slots():
    keys = hm.keys_with_home(5, 128, 20)
    assert len(set(keys)) == 20
    assert all(hm.home_slot(k, 128) == 5 for k in keys)
    more = hm.keys_with_home(5, 128, 5, exclude=keys)
    assert not set(more) & set(keys)
    chain = hm.wrapping_chain(128, 12)
    sim = hm.SlotSim(64)
    at = [sim.insert(k)[0] for k in chain]
    assert at == [(125 + i) % 128 for i in range(12)]     # wraps to slot 0
    one = hm.one_key_per_home(range(128), 128)
    assert sorted(hm.home_slot(k, 128) for k in one) == list(range(128))


def test_model_duplicates_one_winner_and_erase_frees_the_index():
    m = hm.HashModel(4, (2,))
    batch = [(1, 2, 3), (1, 2, 3), (0, 0, 1 << 20), (7, 7, 7), (1, 2, 3)]
    new = m.new_keys(batch)
    assert new == {(1, 2, 3): [0, 1, 4], (7, 7, 7): [3]}   # one winner each
    m.commit_insert((1, 2, 3), 0, [b"ab"])
    m.commit_insert((7, 7, 7), 1, [b"cd"])
    assert m.new_keys(batch) == {} and m.size() == 2
    with pytest.raises(AssertionError):
        m.commit_insert((9, 9, 9), 1, [b"xx"])              # index in use
    mask, idx = m.find(batch)
    assert mask.tolist() == [True, True, False, True, True]
    assert idx.tolist() == [0, 0, 0, 1, 0]
    assert m.present_keys(batch + [(8, 8, 8)]) == \
        {(1, 2, 3): [0, 1, 4], (7, 7, 7): [3]}
    m.commit_erase((7, 7, 7))
    assert m.free == {1, 2, 3} and m.active() == {0} and not m.pristine
    m.commit_insert((9, 9, 9), 1, [b"xx"])                  # free again
    m.reindex(8, {(1, 2, 3): 5, (9, 9, 9): 0})
    assert m.find([(1, 2, 3)])[1].tolist() == [5]
    assert m.entries[(1, 2, 3)][1] == [b"ab"] and len(m.free) == 6
    m.clear()
    assert m.size() == 0 and m.free == set(range(8)) and m.pristine


def test_simulator_first_tombstone_rule_and_rebuild_points():
    sim = hm.SlotSim(64)
    chain = hm.keys_with_home(10, 128, 6)
    assert [sim.insert(k)[0] for k in chain] == [10, 11, 12, 13, 14, 15]
    assert sim.insert(chain[3]) == (13, False)
    assert not sim.erase_batch([chain[1], chain[3]])
    assert sim.tombstones() == [11, 13] and sim.taken == 6
    assert sim.find(chain[5]) == 15                  # behind two tombstones
    assert sim.insert(chain[5]) == (15, False)       # ... and not re-inserted
    new = hm.keys_with_home(10, 128, 1, exclude=chain)[0]
    assert sim.insert(new) == (11, True)             # the FIRST tombstone
    assert sim.taken == 6                            # a tombstone, not empty
    assert sim.find((999, 999, 999)) is None


def test_no_empty_slot_construction():
    plan, crossing = hm.crowding_plan(64)
    for op, keys in plan:
        assert len(set(keys)) == len(keys)
    sim = hm.replay(plan, 64)
    assert sim.n == 128 and sim.empty_slots() == [] and sim.rebuilds == 0
    assert sim.taken == 128 and len(sim.live()) <= 63
    assert len(sim.tombstones()) == 128 - len(sim.live())
    # an absent key: its walk ends only by the bound, a new key takes the
    # first tombstone behind its home slot
    absent = (555, 555, 555)
    assert sim.find(absent) is None
    home = sim.home(absent)
    first_tomb = next((home + i) % 128 for i in range(128)
                      if sim.slots[(home + i) % 128] is sim.TOMB)
    assert sim.insert(absent) == (first_tomb, True)
    live = set(sim.live())
    assert sim.size_call() and sim.rebuilds == 1
    assert set(sim.live()) == live and sim.taken == len(live)
    assert sim.tombstones() == []


def test_crowded_by_inserts_not_by_erase():
    plan, crossing = hm.crowding_plan(64)
    assert [op for op, _ in plan] == ["insert", "erase", "insert", "erase",
                                      "insert"]
    assert crossing == 4
    sim = hm.SlotSim(64)
    for op, keys in plan[:crossing]:
        if op == "insert":
            for k in keys:
                slot, new = sim.insert(k)
                assert new and slot == sim.home(k)    # thread order is moot
        else:
            assert not sim.erase_batch(keys)          # no erase rebuilds
        assert not sim.size_call()                    # nor a size in between
    assert sim.taken == 95 and not sim.crowded()      # one below the mark
    sim.insert(plan[crossing][1][0])
    assert sim.taken == 96 and sim.crowded()          # crossed by an insert
    assert sim.rebuilds == 0
    assert sim.size_call() and sim.rebuilds == 1


# ---- the checker on a plain-Python map ---------------------------------------

class PyMap:
    """A dictionary map behind the driver interface, with the identity heap of
    HashBackendBuffer; `fault` switches one deliberate error on."""

    def __init__(self, capacity, sizes, rng, fault=None):
        self.sizes, self.rng, self.fault = tuple(sizes), rng, fault
        self._alloc(capacity)

    def _alloc(self, capacity):
        self.cap = capacity
        self.d = {}
        self.heap = list(range(capacity))
        self.top = 0
        self.kb = np.zeros((capacity, 3), np.int32)
        self.vb = [np.zeros((capacity, s), np.uint8) for s in self.sizes]

    def capacity(self):
        return self.cap

    def key_buffer(self):
        return self.kb.copy()

    def value_buffer(self, j):
        return self.vb[j].copy()

    def insert(self, keys, rows):
        n = len(keys)
        idx, mask = np.zeros(n, np.int32), np.zeros(n, bool)
        occ = {}
        for i, k in enumerate(keys):
            occ.setdefault(tuple(int(c) for c in k), []).append(i)
        for k, pos in occ.items():
            if not hm.key_in_range(*k) or k in self.d:
                continue
            w = pos[int(self.rng.integers(len(pos)))]
            winners = pos[:2] if self.fault == "two_winners" else [w]
            for w in winners:
                i = self.heap[self.top]
                self.top += 1
                self.d[k] = i
                self.kb[i] = k
                src = pos[0] if self.fault == "row_of_first" else w
                for j in range(len(self.sizes) if rows else 0):
                    self.vb[j][i] = rows[j][src]
                idx[w], mask[w] = i, True
        return idx, mask

    def activate(self, keys):
        return self.insert(keys, None)

    def find(self, keys):
        n = len(keys)
        idx, mask = np.zeros(n, np.int32), np.zeros(n, bool)
        for i, k in enumerate(keys):
            k = tuple(int(c) for c in k)
            if k in self.d:
                idx[i], mask[i] = self.d[k], True
                if self.fault == "find_off_by_one" and self.d[k] > 2:
                    idx[i] -= 1
        return idx, mask

    def erase(self, keys):
        mask = np.zeros(len(keys), bool)
        for i, k in enumerate(keys):
            k = tuple(int(c) for c in k)
            if k in self.d:
                self.top -= 1
                self.heap[self.top] = self.d.pop(k)
                mask[i] = True
            elif self.fault == "erase_all_dups" and i and \
                    any(tuple(int(c) for c in q) == k and mask[p]
                        for p, q in enumerate(keys[:i])):
                mask[i] = True
        return mask

    def size(self):
        return 0, len(self.d)

    def active(self):
        a = np.array(sorted(self.d.values()), np.int32)
        return a[1:] if self.fault == "active_drops_one" and len(a) > 3 else a

    def clear(self):
        self.d = {}
        self.heap = list(range(self.cap))
        self.top = 0

    def reserve(self, capacity):
        if capacity <= len(self.d):
            return 0
        old = [(k, self.kb[i].copy(), [v[i].copy() for v in self.vb])
               for k, i in self.d.items()]
        self._alloc(capacity)
        for n, j in enumerate(self.rng.permutation(len(old))):
            k, _, rows = old[j]
            self.d[k] = n
            self.kb[n] = k
            for a, r in enumerate(rows):
                self.vb[a][n] = r
                if self.fault == "reserve_truncates_row" and len(r) > 1:
                    self.vb[a][n][-1] ^= 1
        self.top = len(old)
        return 0

    def to_device(self):
        o = PyMap(self.cap, self.sizes, self.rng)
        o.reserve_from(self)
        return o

    def reserve_from(self, src):
        for n, (k, i) in enumerate(src.d.items()):
            self.d[k] = n
            self.kb[n] = k
            for a in range(len(self.sizes)):
                self.vb[a][n] = src.vb[a][i]
        self.top = len(src.d)


@pytest.mark.parametrize("capacity", [1, 2, 63, 300])
def test_checker_accepts_a_correct_map(capacity):
    rng = np.random.default_rng(capacity)
    chk = hc.Checker(PyMap(capacity, (4, 3), rng), (4, 3))
    hc.random_stream(chk, rng, 60)
    other = chk.to_device()
    if chk.model.size():
        k = next(iter(chk.model.entries))
        other.erase([k])
        chk.find([k])
        chk.association()


@pytest.mark.parametrize("fault", ["two_winners", "row_of_first",
                                   "find_off_by_one", "erase_all_dups",
                                   "active_drops_one",
                                   "reserve_truncates_row"])
def test_checker_rejects_a_faulty_map(fault):
    rng = np.random.default_rng(3)
    chk = hc.Checker(PyMap(40, (4, 3), rng, fault), (4, 3))
    with pytest.raises(AssertionError):
        hc.random_stream(chk, rng, 200)


def test_packed_model_agrees_with_the_dictionary_model():
    rng = np.random.default_rng(9)
    dev = PyMap(500, (), rng)
    pm = hm.PackedModel(500)
    for step in range(30):
        free = 500 - pm.size()
        keys = rng.integers(-6, 6, size=(int(rng.integers(1, 200)), 3))
        keys = keys.astype(np.int32)
        if step % 3 == 2:
            mask = dev.erase(keys)
            pm.check_erase(keys, mask)
        else:
            ok = ~pm.lookup(hm.pack_keys(keys))[0]
            first = np.unique(hm.pack_keys(keys[ok]), return_index=True)[1]
            drop = np.flatnonzero(ok)[np.sort(first)[free:]]
            keys = keys[~np.isin(hm.pack_keys(keys),
                                 hm.pack_keys(keys[drop]))] if len(drop) \
                else keys
            if not len(keys):
                continue
            idx, mask = dev.activate(keys)
            pm.check_insert(keys, mask, idx, dev.key_buffer())
        idx, mask = dev.find(keys)
        pm.check_find(keys, mask, idx)
        pm.check_active(dev.size()[1], dev.active())
        assert pm.size() == len(dev.d)
        got = dict(zip(map(tuple, hm.unpack_keys(pm.keys).tolist()),
                       pm.idx.tolist()))
        assert got == dev.d
    # a second winner for one key is rejected
    keys = np.array([[50, 50, 50], [50, 50, 50]], np.int32)
    with pytest.raises(AssertionError):
        hm.PackedModel(8).check_insert(keys, [1, 1], [0, 1],
                                       np.array([[50, 50, 50]] * 8))
