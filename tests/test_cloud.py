"""CPU tests of the sets on arbitrary directions (include/jefferson.h: jf_cloud): the triangulation, the host twin
of the kernels' rule against a float64 reference (tests/cloud_model.py: brute force over all triangles, no walk, no seed cells),
continuity across edges, the FD_BASIC pick, the refusals, and a SOFA set of arbitrary directions.  No device is needed: the
host functions are the kernels' own code compiled for the host (csrc/jf_cloud_rule.h); tests/test_gpu_cloud.py holds the device
to them bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import cloud_model
import cloud_sets
from jf_load import jf

HERE = os.path.dirname(os.path.abspath(__file__))
SOFA = os.path.join(HERE, "golden", "sofa")
NAMES = list(cloud_sets.CLOUDS)

# Host twin against float64, dense weight vectors, absolute: 2e-5.  Basis: the error of the number formats -- float32-rounded
# inverses applied to float32 unit vectors, evaluated in NumPy against float64 on the same triangles -- is below 1e-6 on the
# generic and the latitude/longitude cloud and reaches 1.9e-5 on cipic1250 at the positions below (the ears of its 80-degree
# lateral rings: cond of [a b c] up to ~2600), so the library evaluates the direction and lambda in double on the float32 records.
# Measured with that: fib440 1.1e-6, latlong410 2.6e-7, cipic1250 1.1e-5, kemar710 5.1e-6 (printed below with -s).
W_TOL = 2e-5


@pytest.fixture(scope="module")
def clouds():
    out = {}
    for name, fn in cloud_sets.CLOUDS.items():
        azi, ele = fn()
        c = jf.Cloud(azi, ele, 0.05)
        tri = c.triangles()
        out[name] = (c, azi, ele, tri, cloud_model.CloudRef(azi, ele, tri))
    yield out
    for c, *_ in out.values():
        c.close()


def _dense(rows, w, n):
    d = np.zeros((len(rows), n))
    np.add.at(d, (np.arange(len(rows))[:, None], rows), w.astype(np.float64))
    return d


@pytest.mark.parametrize("name", NAMES)
def test_triangulation(clouds, name):
    c, azi, ele, tri, _ = clouds[name]
    n = len(azi)
    assert c.rows() == n and tri.shape == (2 * n - 4, 3)
    assert tri.min() == 0 and tri.max() == n - 1 and len(np.unique(tri)) == n          # every row a vertex
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all()             # from the lowest row on
    # every undirected edge in exactly two faces, once in each direction
    directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    keys = directed[:, 0].astype(np.int64) * n + directed[:, 1]
    assert len(np.unique(keys)) == len(keys) == 3 * (2 * n - 4)
    assert np.array_equal(np.sort(keys), np.sort(directed[:, 1].astype(np.int64) * n + directed[:, 0]))
    # outward, and Delaunay: no direction above any face's plane
    v = cloud_model.unit(azi, ele)
    a, b, cc = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    nrm = np.cross(b - a, cc - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    off = (nrm * a).sum(axis=1)
    assert (off > 0).all()                                                              # the origin strictly inside
    above = (nrm @ v.T - off[:, None]).max()
    print(f"{name}: highest direction above a face's plane {above:.3e}")
    assert above <= 1e-12


def test_fib440_faces_equal_qhulls(clouds):
    spatial = pytest.importorskip("scipy.spatial")
    _, azi, ele, tri, _ = clouds["fib440"]
    hull = spatial.ConvexHull(cloud_model.unit(azi, ele))
    assert {frozenset(t) for t in tri.tolist()} == {frozenset(s) for s in hull.simplices.tolist()}


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_against_float64(clouds, name):
    c, azi, ele, tri, ref = clouds[name]
    n = len(azi)
    pe, pa = cloud_sets.test_positions(name)
    rows, w, nt = c.interpolation_many(pe, pa)
    assert (nt == 3).all() and rows.min() >= 0 and rows.max() < n
    assert (w >= 0).all()
    s = w[:, 0].astype(np.float32) + w[:, 1] + w[:, 2]
    assert np.abs(s.astype(np.float64) - 1.0).max() <= 4 * np.finfo(np.float32).eps
    got, want = _dense(rows, w, n), ref.dense(pe, pa)
    err = np.abs(got - want).max(axis=1)
    print(f"{name}: largest weight difference to float64 {err.max():.3e} over {len(pe)} positions")
    assert err.max() <= W_TOL
    # the rows are a triangle of the triangulation, in its order; the same answer every time
    faces = {tuple(t) for t in tri.tolist()}
    assert all(tuple(r) in faces for r in rows[::97].tolist())
    again = c.interpolation_many(pe[:500], pa[:500])
    assert np.array_equal(again[0], rows[:500]) and np.array_equal(again[1], w[:500])
    # the walk: about two records
    steps = np.array([c.walk(float(e), float(a)) for e, a in zip(pe[:4000], pa[:4000])])
    print(f"{name}: walk mean {steps.mean():.2f} max {steps.max()}")
    assert steps.min() >= 1 and steps.max() < 64


@pytest.mark.parametrize("name", NAMES)
def test_continuity_along_great_circles(clouds, name):
    c, azi, ele, _, ref = clouds[name]
    n = len(azi)
    t = np.radians(np.arange(0.0, 360.0, 0.01))
    frames = [((1, 0, 0), (0, 1, 0)), ((1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)),
              ((0.6, 0.8, 0.0), (-0.48, 0.36, 0.8))]
    worst = 0.0
    for u, v in frames:
        p = np.outer(np.cos(t), u) + np.outer(np.sin(t), v)
        pe = np.degrees(np.arcsin(np.clip(p[:, 2], -1, 1))).astype(np.float32)
        pa = np.mod(np.degrees(np.arctan2(p[:, 0], p[:, 1])), 360.0).astype(np.float32)
        pa[pa >= 360.0] = 0.0
        rows, w, nt = c.interpolation_many(pe, pa)
        assert (nt == 3).all()
        for lo in range(0, len(t), 6000):
            hi = min(len(t), lo + 6001)
            got, want = _dense(rows[lo:hi], w[lo:hi], n), ref.dense(pe[lo:hi], pa[lo:hi])
            excess = np.abs(np.diff(got, axis=0)).max(axis=1) - np.abs(np.diff(want, axis=0)).max(axis=1)
            worst = max(worst, float(excess.max()))
    print(f"{name}: largest step of the weights beyond float64's own {worst:.3e}")
    assert worst <= 2 * W_TOL


@pytest.mark.parametrize("name", NAMES)
def test_pick_is_the_vertex_of_greatest_weight(clouds, name):
    """jf_cloud_pick equals the float64 reference's vertex of greatest weight wherever its two largest weights differ by more
    than 1e-3.  The share of positions that lie nearer to a tie is asserted (< 2 %) over the uniform random directions: the
    constructed positions are ties BY CONSTRUCTION on the ring sets -- the 5-degree lattice puts 432 positions on the midpoints
    of latlong410's meridian edges (weights 1/2, 1/2, 0) and about as many on kemar710's, 1.9 % of all positions by themselves
    (measured over all positions: fib440 0.15 %, latlong410 2.11 %, cipic1250 0.31 %, kemar710 2.19 %) -- so there the pick is
    not left unchecked but held to the vertices whose weight is within 1e-3 of the greatest."""
    c, azi, ele, _, ref = clouds[name]
    pe, pa = cloud_sets.test_positions(name)
    n_random = 20000
    t, w = ref.weights(pe, pa)
    srt = np.sort(w, axis=1)
    clear = srt[:, 2] - srt[:, 1] > 1e-3
    share, share_all = 1.0 - clear[:n_random].mean(), 1.0 - clear.mean()
    print(f"{name}: within 1e-3 of a tie: {100 * share:.2f} % of the random directions, {100 * share_all:.2f} % of all positions")
    assert share < 0.02
    want = ref.tri[t, w.argmax(axis=1)]
    got = np.array([c.pick(float(e), float(a)) for e, a in zip(pe, pa)])
    assert np.array_equal(got[clear], want[clear])
    for i in np.nonzero(~clear)[0]:
        near = ref.tri[t[i]][w[i] >= srt[i, 2] - 1e-3]
        assert got[i] in near, (i, pe[i], pa[i], got[i], near)
    # every vertex picks itself
    assert all(c.pick(float(ele[i]), float(azi[i])) == i for i in range(0, len(azi), 7))


def _refused(azi, ele, tol=0.05):
    with pytest.raises(jf.JfError) as ex:
        jf.Cloud(np.asarray(azi, np.float32), np.asarray(ele, np.float32), tol)
    assert ex.value.code == jf.JF_ERR_ARG and len(str(ex.value).split(": ", 1)[1]) > 0
    return str(ex.value)


def test_refusals(clouds):
    azi, ele = cloud_sets.fib440()
    up = ele >= 0
    assert "hemisphere" in _refused(azi[up], ele[up])
    la, le = cloud_sets.latlong410()
    up = le >= 0                                                                     # the ring at 0 lies in a plane with the origin
    assert "hemisphere" in _refused(la[up], le[up])
    assert "closer" in _refused(np.append(azi, azi[17]), np.append(ele, ele[17]))
    assert "closer" in _refused(np.append(la, 40.0), np.append(le, 90.0))            # the pole a second time
    assert "4" in _refused(azi[:3], ele[:3])
    bad = azi.copy()
    bad[5] = np.nan
    _refused(bad, ele)
    bad = ele.copy()
    bad[9] = np.inf
    _refused(azi, bad)
    bad[9] = 91.0
    _refused(azi, bad)
    big_a, big_e = cloud_sets.fibonacci(16385)
    assert "16384" in _refused(big_a, big_e)
    _refused([0, 90, 180, 270, 45], [0, 0, 0, 0, 0])                                  # one plane
    L = jf.lib()
    h = ctypes.POINTER(jf.JfCloudOpaque)()
    f = azi.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.jf_cloud_create(440, None, f, 0.05, ctypes.byref(h)) == jf.JF_ERR_ARG
    assert L.jf_cloud_create(440, f, f, 0.05, None) == jf.JF_ERR_ARG
    assert L.jf_cloud_rows(None) == jf.JF_ERR_ARG and L.jf_cloud_triangles(None, None) == jf.JF_ERR_ARG
    assert L.jf_cloud_interpolation(None, 0.0, 0.0, None, None) == jf.JF_ERR_ARG
    assert L.jf_cloud_pick(None, 0.0, 0.0) == jf.JF_ERR_ARG
    assert L.jf_sofa_cloud(None, 0.05, None, None, 4) == jf.JF_ERR_ARG
    assert L.jf_engine_create_cloud(None, None, None, 4, None) == jf.JF_ERR_ARG
    assert L.jf_engine_create_sofa_cloud(None, None, 0.05, None) == jf.JF_ERR_ARG
    L.jf_cloud_destroy(None)
    # positions without an answer: no terms, no pick
    c = clouds["fib440"][0]
    for e, a in ((91.0, 0.0), (-90.5, 10.0), (np.nan, 0.0), (0.0, np.nan), (0.0, np.inf), (0.0, 2.0e6)):
        assert c.interpolation(e, a) is None and c.pick(e, a) == jf.JF_ERR_RANGE
    # azimuths fold: -90 is 270, 725 is 5
    for e, a, b in ((10.0, -90.0, 270.0), (-33.5, 725.0, 5.0), (90.0, 123.0, 0.0)):
        r1, r2 = c.interpolation(e, a), c.interpolation(e, b)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    # the ring door still refuses a set that is not rings
    with pytest.raises(jf.JfError) as ex:
        jf.Grid.from_positions(azi, ele)
    assert ex.value.code == jf.JF_ERR_ARG


def test_a_large_cloud_and_the_limit():
    """16 384 directions, the limit: triangulated, every face outward, the twin answers"""
    azi, ele = cloud_sets.fibonacci(16384)
    c = jf.Cloud(azi, ele, 0.05)
    tri = c.triangles()
    assert tri.shape == (2 * 16384 - 4, 3) and len(np.unique(tri)) == 16384
    rows, w, nt = c.interpolation_many(ele[::64] * 0.99, azi[::64] + 0.3)
    assert (nt == 3).all() and (w >= 0).all()
    c.close()


def _patched_symtab(tmp_path, name, azi, ele):
    """symtab.sofa holds SourcePosition as one contiguous float64 run of 33 x 3 (the byte string occurs exactly once): all 33
    rows replaced, azimuths written counter-clockwise as SOFA has them"""
    exp = np.load(os.path.join(SOFA, "sofa_expected.npz"))
    raw = open(os.path.join(SOFA, "symtab.sofa"), "rb").read()
    old = np.stack([exp["az_sofa"], exp["el"], np.full(33, 1.4)], axis=1).tobytes()
    assert raw.count(old) == 1
    az_sofa = np.mod(360.0 - azi.astype(np.float64), 360.0)
    p = tmp_path / name
    p.write_bytes(raw.replace(old, np.stack([az_sofa, ele.astype(np.float64), np.full(33, 1.4)], axis=1).tobytes()))
    return str(p), exp


def test_sofa_set_of_arbitrary_directions(tmp_path):
    """A SOFA file whose 33 directions are a Fibonacci sphere goes through the cloud door: rows in file order, azimuths
    converted, the file's impulse responses.  The ring door's refusal is shown on a second file: 33 directions at 33 different
    elevations ARE a grid to jf_grid_from_positions -- 33 rings of one measurement, within JF_MAX_RINGS -- so the Fibonacci
    file itself is not refused by jf_sofa_table; with two of its directions moved to one elevation (a ring of two that is not
    at 0 / 180 degrees) the set is "not a grid of rings", JF_ERR_ARG as before, and still a cloud."""
    azi, ele = cloud_sets.fibonacci(33)
    p, exp = _patched_symtab(tmp_path, "fib33.sofa", azi, ele)
    s = jf.SofaSet(p)
    cloud, hrir = s.cloud()
    assert cloud.rows() == 33 and hrir.shape == (33, 2, 24)
    assert np.array_equal(hrir, exp["ir"])                                           # file order
    conv = np.float32(360.0) - s.azimuth                                             # azimuths converted as jf_sofa_table converts
    conv[conv >= 360.0] -= np.float32(360.0)
    assert np.abs(conv - azi).max() < 1e-4
    direct = jf.Cloud(conv, s.elevation, 0.05)                                        # the same cloud
    assert np.array_equal(cloud.triangles(), direct.triangles())
    for e, a in ((12.5, 40.0), (-70.0, 200.0), (88.0, 359.5)):
        r1, r2 = cloud.interpolation(e, a), direct.interpolation(e, a)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    s.close()
    ele2 = ele.copy()
    ele2[11] = ele2[10]
    p2, _ = _patched_symtab(tmp_path, "fib33_ring_of_two.sofa", azi, ele2)
    s = jf.SofaSet(p2)
    with pytest.raises(jf.JfError) as ex:
        s.table()
    assert ex.value.code == jf.JF_ERR_ARG
    cloud2, hrir2 = s.cloud()
    assert cloud2.rows() == 33 and np.array_equal(hrir2, exp["ir"])
    assert cloud2.triangles().shape == (62, 3)
    s.close()
