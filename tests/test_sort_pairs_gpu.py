"""o3dmi_sort_pairs_u32 against np.argsort(kind="stable"): the sorted pairs are
the stable order of the keys' low key_bits bits, bit for bit, at the tile and
digit edges of the sort."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 8192   # kPairSortTile (csrc/sort.h): elements a block owns
DIGIT = 8     # kPairSortBits (csrc/sort.h): the widest digit of a pass

SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 100003]
KEY_BITS = [1, DIGIT, DIGIT + 1, 16, 17, 32]
PATTERNS = ["equal", "ascending", "descending", "high_bits_only", "random"]


def _L():
    from open3d_amd import _lib
    return _lib


def _keys(pattern, n, key_bits, rng):
    span = 1 << key_bits
    if pattern == "equal":
        return np.full(n, 0x5A5A5A5A, np.uint32)
    if pattern == "ascending":
        return (np.arange(n, dtype=np.uint64) % span).astype(np.uint32)
    if pattern == "descending":
        return (np.arange(n, dtype=np.int64)[::-1] % span).astype(np.uint32)
    if pattern == "high_bits_only":
        # only bits above key_bits differ: the order must be left alone
        # (key_bits == 32 has no such bits: every key is then equal)
        low = np.uint64(0x2B & (span - 1))
        high = rng.integers(0, 1 << 32, n, dtype=np.uint64) >> \
            np.uint64(key_bits) << np.uint64(key_bits)
        return ((high & np.uint64(0xFFFFFFFF)) | low).astype(np.uint32)
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _sort(keys, vals, key_bits):
    L = _L()
    k = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    v = torch.from_numpy(vals.view(np.int32).copy()).cuda()
    st = L.lib().o3dmi_sort_pairs_u32(L.ptr(k), L.ptr(v), len(keys), key_bits,
                                      None)
    torch.cuda.synchronize()
    return st, k.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("n", SIZES)
def test_sort_pairs_is_the_stable_order(n, key_bits):
    rng = np.random.default_rng(1000 * key_bits + n)
    for pattern in PATTERNS:
        keys = _keys(pattern, n, key_bits, rng)
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        st, k, v = _sort(keys, vals, key_bits)
        assert st == 0, pattern
        mask = np.uint32((1 << key_bits) - 1)
        order = np.argsort(keys & mask, kind="stable")
        assert np.array_equal(k, keys[order]), pattern
        assert np.array_equal(v, vals[order]), pattern
        if pattern in ("equal", "high_bits_only"):
            assert np.array_equal(v, vals), pattern  # input order


def test_sort_pairs_arguments():
    L = _L()
    k = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((None, L.ptr(k), 4, 8), (L.ptr(k), None, 4, 8),
                 (L.ptr(k), L.ptr(k), -1, 8), (L.ptr(k), L.ptr(k), 4, 33),
                 (L.ptr(k), L.ptr(k), 4, -1),
                 (L.ptr(k), L.ptr(k), 1 << 31, 8)):
        assert L.lib().o3dmi_sort_pairs_u32(*args, None) == 1, args
    # key_bits == 0: nothing is told apart, nothing moves
    keys = np.array([3, 1, 2], np.uint32)
    st, kk, vv = _sort(keys, keys.copy(), 0)
    assert st == 0 and kk.tolist() == [3, 1, 2] and vv.tolist() == [3, 1, 2]


def test_sort_pairs_same_bits_every_run():
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 50, 3 * TILE + 17, dtype=np.uint64) \
        .astype(np.uint32)
    vals = np.arange(len(keys), dtype=np.uint32)
    first = _sort(keys, vals, 6)
    second = _sort(keys, vals, 6)
    assert np.array_equal(first[1], second[1])
    assert np.array_equal(first[2], second[2])
