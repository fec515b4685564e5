"""GPU tests of the ray queries on a mesh (CastRays, TestOcclusions,
CountIntersections, ListIntersections, ComputeOccupancy,
ComputeSignedDistance, CreateRaysPinhole) against the numpy restatement
(tests/_mesh_ray_oracle.py: exhaustive loops, it never builds a tree) and
upstream's literal vectors (tests/golden/raycasting_vectors.json). Every
comparison is bit for bit unless a tolerance is named; outputs are poisoned
first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _mesh_ray_oracle as orc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, 1, 3, 7
F32C, F64C, I32C, I64C = 0, 1, 4, 5
F32 = np.float32
INF = float("inf")
POISON = -777.0
POISON_ID = 0x5A5A5A5A
POISON_COUNT = -77
POISON_BYTE = 0x5A
CLOSEST, ANY, COUNT = 0, 1, 2
CAST_KEYS = ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs",
             "primitive_normals")
LIST_KEYS = ("ray_ids", "t_hit", "geometry_ids", "primitive_ids",
             "primitive_uvs")
TCODE = {torch.float32: F32C, torch.float64: F64C, torch.int32: I32C,
         torch.int64: I64C}


def _L():
    from open3d_amd import _lib
    return _lib


def _tm():
    from open3d_amd import trianglemesh
    return trianglemesh


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32,
                   8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.size == 0:
        return
    differ = (_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1)
    bad = np.flatnonzero(differ)
    assert len(bad) == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _mesh_args(p, t):
    L = _L()
    return (L.ptr(p), p.shape[0], TCODE[p.dtype], L.ptr(t), t.shape[0],
            TCODE[t.dtype])


def _poisoned(key, rows):
    rows = max(rows, 1)
    if key in ("geometry_ids", "primitive_ids"):
        return torch.full((rows,), POISON_ID, dtype=torch.int32,
                          device="cuda")
    if key == "ray_ids":
        return torch.full((rows,), POISON_COUNT, dtype=torch.int64,
                          device="cuda")
    shape = {"primitive_uvs": (rows, 2), "primitive_normals": (rows, 3)}.get(
        key, (rows,))
    return torch.full(shape, POISON, dtype=torch.float32, device="cuda")


def _numpy(tensors, rows):
    out = {}
    for k, v in tensors.items():
        a = v.cpu().numpy()
        if k in ("geometry_ids", "primitive_ids"):
            a = a.view(np.uint32)
        out[k] = a[:rows]
    return out


def _untouched(out):
    for k, a in out.items():
        if k in ("geometry_ids", "primitive_ids"):
            assert (a == POISON_ID).all(), k
        elif k == "ray_ids":
            assert (a == POISON_COUNT).all(), k
        else:
            assert (a == POISON).all(), k


class Scene:
    def __init__(self, pos, tri):
        self.pos, self.tri = np.asarray(pos, F32), np.asarray(tri)
        self.pd, self.td = _dev(self.pos), _dev(self.tri)
        self.h = C.c_void_p()
        self.status = _L().lib().o3dmi_mesh_bvh_create(
            *_mesh_args(self.pd, self.td), C.byref(self.h), None)
        assert self.status == OK

    def cast(self, rays, order=None, tnear=0.0, tfar=INF, keys=CAST_KEYS,
             code=F32C, visits=None):
        """order None: the public call; 0 / 1: the internal call with the rays
        in input / Morton order. keys: the outputs that are not NULL."""
        L = _L()
        rays = np.asarray(rays)
        rd, q = _dev(rays), len(rays)
        t = {k: _poisoned(k, q) for k in keys}
        ptrs = [L.ptr(t.get(k)) for k in CAST_KEYS]
        if order is None:
            st = L.lib().o3dmi_mesh_bvh_cast_rays(self.h, L.ptr(rd), q, code,
                                                  *ptrs, None)
        else:
            st = L.lib().o3dmi_internal_mesh_bvh_ray_query(
                self.h, CLOSEST, L.ptr(rd), q, tnear, tfar, *ptrs, None, None,
                order, visits, None)
        return st, _numpy(t, q)

    def occluded(self, rays, tnear=0.0, tfar=INF, order=None, code=F32C):
        L = _L()
        rays = np.asarray(rays)
        rd, q = _dev(rays), len(rays)
        out = torch.full((max(q, 1),), POISON_BYTE, dtype=torch.uint8,
                         device="cuda")
        if order is None:
            st = L.lib().o3dmi_mesh_bvh_test_occlusions(
                self.h, L.ptr(rd), q, code, tnear, tfar, L.ptr(out), None)
        else:
            st = L.lib().o3dmi_internal_mesh_bvh_ray_query(
                self.h, ANY, L.ptr(rd), q, tnear, tfar, None, None, None,
                None, None, L.ptr(out), None, order, None, None)
        return st, out.cpu().numpy()[:q]

    def count(self, rays, order=None, code=F32C):
        L = _L()
        rays = np.asarray(rays)
        rd, q = _dev(rays), len(rays)
        out = torch.full((max(q, 1),), POISON_COUNT, dtype=torch.int32,
                         device="cuda")
        if order is None:
            st = L.lib().o3dmi_mesh_bvh_count_intersections(
                self.h, L.ptr(rd), q, code, L.ptr(out), None)
        else:
            st = L.lib().o3dmi_internal_mesh_bvh_ray_query(
                self.h, COUNT, L.ptr(rd), q, 0.0, INF, None, None, None, None,
                None, None, L.ptr(out), order, None, None)
        return st, out.cpu().numpy()[:q]

    def list(self, rays, capacity, keys=LIST_KEYS, rows=None, splits=True,
             code=F32C):
        """-> status, total, ray_splits (or None), the entry arrays with
        `rows` rows (default: the capacity)."""
        L = _L()
        rays = np.asarray(rays)
        rd, q = _dev(rays), len(rays)
        rows = max(capacity, 0) if rows is None else rows
        sp = torch.full((q + 1,), POISON_COUNT, dtype=torch.int64,
                        device="cuda") if splits else None
        t = {k: _poisoned(k, rows) for k in keys}
        total = C.c_int64(POISON_COUNT)
        st = L.lib().o3dmi_mesh_bvh_list_intersections(
            self.h, L.ptr(rd), q, code, L.ptr(sp), capacity, C.byref(total),
            *[L.ptr(t.get(k)) for k in LIST_KEYS], None)
        return (st, total.value, sp.cpu().numpy() if splits else None,
                _numpy(t, max(rows, 1)))

    def vote(self, points, nsamples, signed, code=F32C):
        L = _L()
        points = np.asarray(points)
        pd, q = _dev(points), len(points)
        out = torch.full((max(q, 1),), POISON, dtype=torch.float32,
                         device="cuda")
        fn = L.lib().o3dmi_mesh_bvh_compute_signed_distance if signed else \
            L.lib().o3dmi_mesh_bvh_compute_occupancy
        st = fn(self.h, L.ptr(pd), q, code, nsamples, L.ptr(out), None)
        return st, out.cpu().numpy()[:q]

    def close(self):
        assert _L().lib().o3dmi_mesh_bvh_destroy(self.h) == OK
        self.h = C.c_void_p()


# ---- meshes and rays ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh(name):
    if name in ("m1", "m2", "m3"):
        return orc.soup(int(name[1]), seed=int(name[1]), degenerate_every=0)
    if name == "box":
        return orc.unit_box()
    if name == "soup":  # every fourth triangle degenerate
        return orc.soup(300, seed=11)
    if name == "grid":
        return orc.grid(8)
    if name == "grid2":
        return orc.grid(8, duplicate=True)
    if name == "deep":  # small triangles: a deep tree, long stacks
        rng = np.random.default_rng(12)
        centres = rng.uniform(-1, 1, (5000, 1, 3))
        pos = (centres + 0.08 * rng.standard_normal((5000, 3, 3)))
        return (pos.reshape(-1, 3).astype(F32),
                np.arange(15000, dtype=np.int32).reshape(5000, 3))
    raise KeyError(name)


MESHES = ["m1", "m2", "m3", "box", "soup", "grid", "grid2"]


def mixed_rays(name, q, seed):
    """Rays of every kind the pair function distinguishes, by i % 10."""
    pos, tri = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    size = np.maximum(hi - lo, 1.0)
    rows = []
    for i in range(q):
        kind = i % 10
        t = tri[rng.integers(len(tri))]
        a, b, c = (pos[k].astype(np.float64) for k in t)
        w = rng.dirichlet(np.ones(3))
        on = w[0] * a + w[1] * b + w[2] * c  # a point on a triangle
        o = lo - size + rng.uniform(0, 3, 3) * size
        if kind in (0, 1):  # through a point of the surface, unnormalised
            d = (on - o) * rng.uniform(0.2, 3)
        elif kind == 2:  # axis-parallel, exactly through a mesh vertex
            k = rng.integers(3)
            o = pos[t[rng.integers(3)]].astype(np.float64).copy()
            o[k] = lo[k] - 1.0
            d = np.zeros(3)
            d[k] = rng.choice([0.5, 1.0, 2.0])
        elif kind == 3:  # the origin exactly on the surface (a vertex)
            o = pos[t[rng.integers(3)]].astype(np.float64)
            d = rng.standard_normal(3)
        elif kind == 4:  # very short and very long directions
            d = (on - o) * (1e-20 if i % 20 == 4 else 1e20)
        elif kind == 5:  # zero direction, or pointing away from the scene
            d = np.zeros(3) if i % 20 == 5 else -(size + rng.uniform(0, 1, 3))
            if i % 20 != 5:
                o = lo - size
        elif kind == 6:  # axis-parallel inside the plane of a box face
            k, j = rng.permutation(3)[:2]
            o = pos[t[rng.integers(3)]].astype(np.float64).copy()
            o[j] = lo[j] - 1.0
            d = np.zeros(3)
            d[j] = 1.0  # o_k stays on the vertex's k-plane: lo_k or hi_k
        elif kind == 7:  # along an edge of a triangle, from before it
            o = a - (b - a)
            d = b - a
        elif kind == 8:  # from far outside the scene box, missing it
            o = hi + size * 5
            d = rng.standard_normal(3)
        else:
            d = rng.standard_normal(3)
        rows.append(np.concatenate([o, d]))
    return np.array(rows, np.float64).astype(F32).reshape(q, 6)


@functools.lru_cache(maxsize=None)
def reference(name, q, seed):
    pos, tri = mesh(name)
    rays = mixed_rays(name, q, seed)
    lst = orc.list_intersections(pos, tri, rays)
    return dict(rays=rays, cast=orc.cast_rays(pos, tri, rays),
                occluded=orc.occlusions(pos, tri, rays), list=lst,
                counts=np.diff(lst["ray_splits"]).astype(np.int32))


def check_scene(name, q, seed, orders=(None, 0, 1)):
    want = reference(name, q, seed)
    rays = want["rays"]
    sc = Scene(*mesh(name))
    for order in orders:
        st, got = sc.cast(rays, order)
        assert st == OK
        for k in CAST_KEYS:
            _same(got[k], want["cast"][k], "%s (order %r)" % (k, order))
        st, occ = sc.occluded(rays, order=order)
        assert st == OK
        assert occ.tolist() == want["occluded"].astype(np.uint8).tolist()
        st, counts = sc.count(rays, order)
        assert st == OK
        _same(counts, want["counts"], "counts (order %r)" % (order,))
    total = int(want["counts"].sum())
    st, n, splits, got = sc.list(rays, total)
    assert st == OK and n == total
    _same(splits, want["list"]["ray_splits"], "ray_splits")
    for k in LIST_KEYS:
        _same(got[k][:total], want["list"][k], "list " + k)
    sc.close()
    return want


# ---- the queries against the restatement ---------------------------------------------
@pytest.mark.parametrize("q", [1, 127, 128, 129])
@pytest.mark.parametrize("name", MESHES)
def test_ray_queries_on_small_meshes(name, q):
    want = check_scene(name, q, seed=q)
    if q >= 127 and name not in ("m1", "m2", "m3"):
        assert want["counts"].sum() > 10  # rays that hit, and rays that miss
        assert (want["counts"] == 0).sum() > 10


def test_ray_queries_on_two_thousand_rays():
    want = check_scene("soup", 2003, seed=5)
    assert want["counts"].max() >= 3


def test_ray_queries_on_a_deep_tree():
    pos, tri = mesh("deep")
    want = check_scene("deep", 300, seed=6)
    assert want["counts"].max() >= 3
    # the tree prunes: far fewer pairs tested than the exhaustive loop's
    sc = Scene(pos, tri)
    for order in (0, 1):
        visits = (C.c_uint64 * 2)(0, 0)
        st, got = sc.cast(want["rays"], order, visits=visits)
        assert st == OK
        _same(got["t_hit"], want["cast"]["t_hit"])
        assert 0 < visits[0] and 0 < visits[1] < 300 * len(tri) // 10
    sc.close()


def test_duplicates_tie_to_the_lowest_index_and_count_once():
    single = reference("grid", 129, 129)
    rays = single["rays"]
    sc = Scene(*mesh("grid2"))  # triangle k of the grid is 2 k and 2 k + 1
    hit = single["cast"]["primitive_ids"] != orc.INVALID_ID
    assert hit.sum() > 10
    for order in (0, 1):
        st, counts = sc.count(rays, order)
        assert st == OK
        _same(counts, single["counts"], "counts")
        st, got = sc.cast(rays, order)
        assert st == OK
        _same(got["t_hit"], single["cast"]["t_hit"], "t_hit")
        assert (got["primitive_ids"][hit] ==
                2 * single["cast"]["primitive_ids"][hit]).all()
        assert (got["primitive_ids"][~hit] == orc.INVALID_ID).all()
    total = int(single["counts"].sum())
    st, n, splits, lst = sc.list(rays, total)
    assert st == OK and n == total
    _same(lst["t_hit"][:total], single["list"]["t_hit"], "list t_hit")
    assert (lst["primitive_ids"][:total] ==
            2 * single["list"]["primitive_ids"]).all()
    sc.close()


def test_range_ends_are_open_below_and_closed_above():
    pos = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
    sc = Scene(pos, np.array([[0, 1, 2]], np.int32))
    rays = np.array([[1, 1, 2, 0, 0, -1],       # t = 2
                     [1, 1, 0, 0, 0, -1],       # starts on the surface
                     [1, 1, -3, 0, 0, 0.5]], F32)  # t = 6
    cases = [(0.0, INF, [1, 0, 1]), (0.0, 2.0, [1, 0, 0]),
             (2.0, INF, [0, 0, 1]), (2.0, 6.0, [0, 0, 1]),
             (6.0, INF, [0, 0, 0]), (-1.0, INF, [1, 1, 1]),
             (INF, INF, [0, 0, 0]), (-INF, -INF, [0, 0, 0])]
    for tnear, tfar, want in cases:
        for order in (None, 0, 1):
            st, occ = sc.occluded(rays, tnear, tfar, order)
            assert st == OK and occ.tolist() == want, (tnear, tfar, order)
        assert orc.occlusions(pos, [[0, 1, 2]], rays, tnear,
                              tfar).tolist() == [bool(x) for x in want]
        st, got = sc.cast(rays, 0, tnear, tfar)
        ref = orc.cast_rays(pos, [[0, 1, 2]], rays, tnear, tfar)
        assert st == OK
        for k in CAST_KEYS:
            _same(got[k], ref[k], k)
    st, got = sc.cast(rays)
    assert got["t_hit"].tolist() == [2.0, INF, 6.0]
    assert got["primitive_ids"].tolist() == [0, orc.INVALID_ID, 0]
    sc.close()


@pytest.mark.parametrize("key", CAST_KEYS)
def test_cast_rays_with_one_output(key):
    want = reference("soup", 129, 129)
    sc = Scene(*mesh("soup"))
    for order in (None, 1):
        st, got = sc.cast(want["rays"], order, keys=(key,))
        assert st == OK and list(got) == [key]
        _same(got[key], want["cast"][key], key)
    st, got = sc.cast(want["rays"], keys=())
    assert st == OK and got == {}
    sc.close()


# ---- purity ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "grid2", "deep"])
def test_a_permuted_mesh_gives_the_same_answers(name):
    pos, tri = mesh(name)
    q = 300 if name == "deep" else 129
    want = reference(name, q, 6 if name == "deep" else q)
    rays = want["rays"]
    perm = np.random.default_rng(7).permutation(len(tri))
    sc = Scene(pos, tri[perm])  # new triangle k is old triangle perm[k]
    st, got = sc.cast(rays)
    assert st == OK
    _same(got["t_hit"], want["cast"]["t_hit"], "t_hit")
    st, counts = sc.count(rays)
    _same(counts, want["counts"], "counts")
    total = int(counts.sum())
    st, n, splits, lst = sc.list(rays, total)
    assert st == OK and n == total
    _same(splits, want["list"]["ray_splits"])
    _same(lst["t_hit"][:total], want["list"]["t_hit"], "list t_hit")
    # where one triangle alone has the closest t, it is the same triangle
    hit, t, _, _ = orc.pairs(pos, tri, rays)
    best = want["cast"]["t_hit"]
    alone = (hit & (t == best[:, None])).sum(axis=1) == 1
    assert alone.sum() > 10 or name == "grid2"  # its triangles come in twos
    mapped = perm[got["primitive_ids"][alone].astype(np.int64)]
    assert mapped.tolist() == want["cast"]["primitive_ids"][alone].tolist()
    sc.close()


def test_the_one_shot_forms_give_the_handles_bits():
    L = _L()
    pos, tri = mesh("soup")
    want = reference("soup", 129, 129)
    pd, td, rd = _dev(pos), _dev(tri.astype(np.int64)), _dev(want["rays"])
    t = {k: _poisoned(k, 129) for k in CAST_KEYS}
    st = L.lib().o3dmi_trianglemesh_cast_rays(
        *_mesh_args(pd, td), L.ptr(rd), 129,
        *[L.ptr(t[k]) for k in CAST_KEYS], None)
    assert st == OK
    got = _numpy(t, 129)
    for k in CAST_KEYS:
        _same(got[k], want["cast"][k], k)
    points = vote_points("soup")
    sc = Scene(pos, tri)
    for nsamples in (1, 3):
        st, handle = sc.vote(points, nsamples, signed=True)
        assert st == OK
        out = _poisoned("t_hit", len(points))
        st = L.lib().o3dmi_trianglemesh_compute_signed_distance(
            *_mesh_args(pd, td), L.ptr(_dev(points)), len(points), nsamples,
            L.ptr(out), None)
        assert st == OK
        _same(out.cpu().numpy(), handle, "signed distance")
    sc.close()


# ---- list ------------------------------------------------------------------------------
def test_list_counting_capacity_and_absent_outputs():
    want = reference("soup", 129, 129)
    rays, ref = want["rays"], want["list"]
    total = int(want["counts"].sum())
    assert total > 20
    sc = Scene(*mesh("soup"))
    # counting mode: the splits and the total, nothing else
    st, n, splits, got = sc.list(rays, -1, rows=total)
    assert st == OK and n == total
    _same(splits, ref["ray_splits"])
    _untouched(got)
    # without the splits
    st, n, splits, got = sc.list(rays, -1, rows=total, splits=False)
    assert st == OK and n == total and splits is None
    # too small: CAPACITY, nothing but the total and the splits written
    for capacity in (0, 1, total - 1):
        st, n, splits, got = sc.list(rays, capacity, rows=total)
        assert st == CAPACITY and n == total
        _same(splits, ref["ray_splits"])
        _untouched(got)
    # exact and generous capacities; the rows past the total stay
    for capacity in (total, total + 5):
        st, n, splits, got = sc.list(rays, capacity)
        assert st == OK and n == total
        for k in LIST_KEYS:
            _same(got[k][:total], ref[k], k)
        _untouched({k: v[total:] for k, v in got.items()})
    # every entry array alone, and none
    for key in LIST_KEYS:
        st, n, splits, got = sc.list(rays, total, keys=(key,), splits=False)
        assert st == OK and n == total and list(got) == [key]
        _same(got[key][:total], ref[key], key)
    st, n, splits, got = sc.list(rays, total, keys=())
    assert st == OK and n == total
    _same(splits, ref["ray_splits"])
    sc.close()


def test_list_with_zero_total():
    sc = Scene(*mesh("box"))
    rays = np.array([[5, 5, 5, 1, 0, 0], [5, 5, 5, 0, 0, 0],
                     [0.5, 0.5, 2, 0, 0, 1]], F32)
    for capacity in (-1, 0, 4):
        st, n, splits, got = sc.list(rays, capacity, rows=4)
        assert st == OK and n == 0
        assert splits.tolist() == [0, 0, 0, 0]
        _untouched(got)
    sc.close()


# ---- the vote ---------------------------------------------------------------------------
def vote_points(name):
    if name == "box":  # inside, outside, on the surface, on edges and corners
        grid = [[x, y, z] for x in (-0.5, 0, 0.25, 0.5, 1, 1.5)
                for y in (-0.5, 0, 0.5, 1) for z in (0, 0.5, 1, 1.25)]
        rng = np.random.default_rng(8)
        return np.concatenate(
            [np.array(grid), rng.uniform(-0.5, 1.5, (60, 3))]).astype(F32)
    return np.random.default_rng(9).uniform(-1.2, 1.2, (130, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def vote_reference(name, nsamples):
    pos, tri = mesh(name)
    points = vote_points(name)
    return (orc.compute_occupancy(pos, tri, points, nsamples),
            orc.compute_signed_distance(pos, tri, points, nsamples))


# 1 and 3: a lane and three lanes a point; 9: more rays than the eight lanes
# a point gets, so a lane takes two of them
@pytest.mark.parametrize("nsamples", [1, 3, 9])
@pytest.mark.parametrize("name", ["box", "soup", "m1"])
def test_occupancy_and_signed_distance(name, nsamples):
    pos, tri = mesh(name)
    points = vote_points(name)
    occ, sd = vote_reference(name, nsamples)
    sc = Scene(pos, tri)
    st, got = sc.vote(points, nsamples, signed=False)
    assert st == OK
    _same(got, occ, "occupancy")
    st, got = sc.vote(points, nsamples, signed=True)
    assert st == OK
    _same(got, sd, "signed distance")
    # the magnitude is the closest-point query's distance, bit for bit
    L = _L()
    dist = _poisoned("t_hit", len(points))
    assert L.lib().o3dmi_mesh_bvh_closest_points(
        sc.h, L.ptr(_dev(points)), len(points), F32C, None, None, None, None,
        L.ptr(dist), None) == OK
    _same(np.abs(got), dist.cpu().numpy(), "|signed distance|")
    if name == "box":
        assert 0 < occ.sum() < len(occ)
        assert (sd[occ == 1] <= 0).all() and (sd[occ == 0] >= 0).all()
        inside = ((points > 0) & (points < 1)).all(axis=1)
        beyond = ((points < 0) | (points > 1)).any(axis=1)
        assert inside.sum() > 10 and beyond.sum() > 10
        assert (occ[inside] == 1).all() and (occ[beyond] == 0).all()
    sc.close()


def test_vote_refuses_even_and_non_positive_nsamples():
    sc = Scene(*mesh("box"))
    points = vote_points("box")[:5]
    for signed in (False, True):
        for bad in (0, 2, 4, -1):
            st, got = sc.vote(points, bad, signed)
            assert st == INVALID_ARG and (got == POISON).all()
    sc.close()


# ---- errors -----------------------------------------------------------------------------
def test_non_finite_input_is_refused_with_the_outputs_untouched():
    sc = Scene(*mesh("box"))
    base = mixed_rays("box", 130, 1)
    for slot in range(6):
        for value in (np.nan, np.inf, -np.inf):
            rays = base.copy()
            rays[(37 * slot + 5) % 130, slot] = value
            st, got = sc.cast(rays)
            assert st == INVALID_ARG
            _untouched(got)
            st, occ = sc.occluded(rays)
            assert st == INVALID_ARG and (occ == POISON_BYTE).all()
            st, counts = sc.count(rays)
            assert st == INVALID_ARG and (counts == POISON_COUNT).all()
            st, n, splits, lst = sc.list(rays, 500)
            assert st == INVALID_ARG and n == POISON_COUNT
            assert (splits == POISON_COUNT).all()
            _untouched(lst)
    for tnear, tfar in ((np.nan, 1.0), (0.0, np.nan)):
        st, occ = sc.occluded(base, tnear, tfar)
        assert st == INVALID_ARG and (occ == POISON_BYTE).all()
        st, got = sc.cast(base, 0, tnear, tfar)
        assert st == INVALID_ARG
        _untouched(got)
    points = vote_points("box")[:10].copy()
    points[3, 1] = np.nan
    for signed in (False, True):
        st, got = sc.vote(points, 1, signed)
        assert st == INVALID_ARG and (got == POISON).all()
    sc.close()


def test_float64_is_unsupported_and_no_rays_are_fine():
    sc = Scene(*mesh("box"))
    rays = mixed_rays("box", 4, 1)
    st, got = sc.cast(rays.astype(np.float64), code=F64C)
    assert st == UNSUPPORTED
    _untouched(got)
    st, occ = sc.occluded(rays.astype(np.float64), code=F64C)
    assert st == UNSUPPORTED and (occ == POISON_BYTE).all()
    st, counts = sc.count(rays.astype(np.float64), code=F64C)
    assert st == UNSUPPORTED and (counts == POISON_COUNT).all()
    st, n, splits, lst = sc.list(rays.astype(np.float64), 10, code=F64C)
    assert st == UNSUPPORTED and n == POISON_COUNT
    _untouched(lst)
    for signed in (False, True):
        st, got = sc.vote(rays[:, :3].astype(np.float64), 1, signed,
                          code=F64C)
        assert st == UNSUPPORTED and (got == POISON).all()
    # q == 0: OK, nothing written
    empty = np.zeros((0, 6), F32)
    for order in (None, 0, 1):
        st, got = sc.cast(empty, order)
        assert st == OK
        st, occ = sc.occluded(empty, order=order)
        assert st == OK
        st, counts = sc.count(empty, order)
        assert st == OK
    st, n, splits, lst = sc.list(empty, 3, rows=3)
    assert st == OK and n == 0 and splits.tolist() == [0]
    _untouched(lst)
    for signed in (False, True):
        st, got = sc.vote(np.zeros((0, 3), F32), 3, signed)
        assert st == OK
    sc.close()


# ---- the pinhole rays ---------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(1, 1), (3, 2), (64, 48)])
def test_create_rays_pinhole(width, height):
    k = np.array([[52.5, 0.25, width / 2 - 0.3], [0, 51.75, height / 2 + 0.2],
                  [0, 0, 1]])
    angle = 0.3
    e = np.eye(4)
    e[:3, :3] = [[np.cos(angle), 0, np.sin(angle)], [0, 1, 0],
                 [-np.sin(angle), 0, np.cos(angle)]]
    e[:3, 3] = [0.1, -0.2, 2.5]
    want = orc.create_rays_pinhole(k, e, width, height)
    L = _L()
    out = torch.full((height, width, 6), POISON, dtype=torch.float32,
                     device="cuda")
    kk, ee = np.ascontiguousarray(k), np.ascontiguousarray(e)
    assert L.lib().o3dmi_create_rays_pinhole(
        L.f64p(kk), L.f64p(ee), width, height, L.ptr(out), None) == OK
    _same(out.cpu().numpy().reshape(-1, 6), want.reshape(-1, 6), "rays")
    got = _tm().create_rays_pinhole(torch.from_numpy(k), e.tolist(), width,
                                    height)
    assert tuple(got.shape) == (height, width, 6)
    _same(got.cpu().numpy().reshape(-1, 6), want.reshape(-1, 6), "mirror")
    # the centre pixel's ray looks along the camera's z axis, from C
    np.testing.assert_allclose(want[0, 0, :3], -e[:3, :3].T @ e[:3, 3],
                               rtol=1e-6)


# ---- upstream's vectors ---------------------------------------------------------------------
def _num(x):
    return np.inf if x == "inf" else x


def test_upstream_vectors_through_the_c_abi():
    gold = orc.golden()
    g = gold["triangle"]
    sc = Scene(np.array(g["positions"], F32),
               np.array(g["triangles"], np.int32))
    rays = np.array(g["rays"], F32)
    st, got = sc.cast(rays)
    assert st == OK
    assert got["geometry_ids"].tolist() == g["cast_rays"]["geometry_ids"]
    assert got["geometry_ids"][1] == gold["invalid_id"]
    assert np.isclose(got["t_hit"][0], g["cast_rays"]["t_hit"][0],
                      rtol=g["cast_rays"]["t_hit_rtol"],
                      atol=g["cast_rays"]["t_hit_atol"])
    assert np.isinf(got["t_hit"][1])
    for case in g["occlusions"]:
        st, occ = sc.occluded(rays, _num(case["tnear"]), _num(case["tfar"]))
        assert st == OK and occ.astype(bool).tolist() == case["occluded"]
    sc.close()
    g = gold["box"]
    sc = Scene(*orc.unit_box())
    rays = np.array(g["rays"], F32)
    st, counts = sc.count(rays)
    assert st == OK and counts.tolist() == g["counts"]
    st, n, splits, lst = sc.list(rays, 3)
    assert st == OK and n == 3
    np.testing.assert_allclose(lst["t_hit"], g["list_t_hit"],
                               rtol=g["list_tolerance"],
                               atol=g["list_tolerance"])
    st, sd = sc.vote(np.array(g["signed_distance_queries"], F32), 1, True)
    assert st == OK
    np.testing.assert_allclose(sd, g["signed_distance"],
                               rtol=g["signed_distance_rtol"])
    st, occ = sc.vote(np.array(g["occupancy_queries"], F32), 1, False)
    assert st == OK and occ.tolist() == g["occupancy"]
    sc.close()


def test_upstream_vectors_through_mesh_bvh():
    tm = _tm()
    gold = orc.golden()
    assert tm.INVALID_ID == gold["invalid_id"]
    g = gold["triangle"]
    bvh = tm.MeshBVH({"positions": _dev(np.array(g["positions"], F32)),
                      "indices": _dev(np.array(g["triangles"], np.int64))})
    rays = _dev(np.array(g["rays"], F32))
    ans = bvh.cast_rays(rays)
    assert ans["geometry_ids"].cpu().numpy().view(np.uint32).tolist() == \
        g["cast_rays"]["geometry_ids"]
    assert np.isclose(ans["t_hit"][0].item(), 1.0)
    assert np.isinf(ans["t_hit"][1].item())
    assert bvh.test_occlusions(rays).tolist() == [True, False]
    assert not bvh.test_occlusions(rays, tfar=0.5).any()
    assert not bvh.test_occlusions(rays, tnear=1.5).any()
    # the output shapes
    s = gold["output_shapes"]
    rs = np.random.RandomState(s["random_state"])
    for shape in s["shapes"]:
        r = _dev(rs.uniform(size=shape + [6]).astype(F32))
        p = _dev(rs.uniform(size=shape + [3]).astype(F32))
        counts = bvh.count_intersections(r)
        assert list(counts.shape) == shape and counts.dtype == torch.int32
        assert list(bvh.compute_distance(p).shape) == shape
        assert list(bvh.compute_signed_distance(p).shape) == shape
        assert list(bvh.compute_occupancy(p).shape) == shape
        assert list(bvh.test_occlusions(r).shape) == shape
        for k, v in bvh.cast_rays(r).items():
            assert list(v.shape) == shape + s["last_dim"][k], k
        for k, v in bvh.compute_closest_points(p).items():
            assert list(v.shape) == shape + s["last_dim"][k], k
        nx = int(counts.sum().item())
        for k, v in bvh.list_intersections(r).items():
            first = int(np.prod(shape)) + 1 if k == "ray_splits" else nx
            assert list(v.shape) == [first] + s["last_dim"][k], k
    bvh.close()
    g = gold["box"]
    pos, tri = orc.unit_box()
    bvh = tm.MeshBVH({"positions": _dev(pos), "indices": _dev(tri)})
    rays = _dev(np.array(g["rays"], F32))
    assert bvh.count_intersections(rays).tolist() == g["counts"]
    lst = bvh.list_intersections(rays)
    np.testing.assert_allclose(lst["t_hit"].cpu().numpy(), g["list_t_hit"],
                               rtol=g["list_tolerance"],
                               atol=g["list_tolerance"])
    assert lst["ray_splits"].tolist() == [0, 2, 3, 3]
    assert lst["ray_ids"].tolist() == [0, 0, 1]
    for nsamples in (1, 3):
        sd = bvh.compute_signed_distance(
            _dev(np.array(g["signed_distance_queries"], F32)), nsamples)
        np.testing.assert_allclose(sd.cpu().numpy(), g["signed_distance"],
                                   rtol=g["signed_distance_rtol"])
        occ = bvh.compute_occupancy(
            _dev(np.array(g["occupancy_queries"], F32)), nsamples=nsamples)
        assert occ.tolist() == g["occupancy"]
    with pytest.raises(_L().O3DMIError):
        bvh.compute_occupancy(_dev(np.zeros((2, 3), F32)), nsamples=2)
    bvh.close()
