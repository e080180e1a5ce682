"""Test clouds for the sets on arbitrary directions (include/jefferson.h: jf_cloud), all from closed formulas: (azimuth, elevation)
in degrees as float32, azimuths in the engine's sense (90 = right).  Checked with SciPy's Qhull: each gives exactly 2n - 4 hull
faces, every direction a hull vertex, the origin strictly inside."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fibonacci(n):
    """Fibonacci sphere: generic position, no degeneracy"""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    azi = np.mod(i * (180.0 * (3.0 - np.sqrt(5.0))), 360.0)
    return azi.astype(np.float32), np.degrees(np.arcsin(z)).astype(np.float32)


def fib440():
    return fibonacci(440)


def latlong410():
    """15 x 10 degrees from -80 to 80 plus both poles: coplanar quads everywhere"""
    ele, azi = np.meshgrid(np.arange(-80.0, 81.0, 10.0), np.arange(0.0, 360.0, 15.0), indexing="ij")
    ele = np.concatenate([[-90.0], ele.ravel(), [90.0]])
    azi = np.concatenate([[0.0], azi.ravel(), [0.0]])
    return azi.astype(np.float32), ele.astype(np.float32)


CIPIC_LATERAL = [-80, -65, -55] + list(range(-45, 50, 5)) + [55, 65, 80]


def cipic1250():
    """interaural-polar: 25 lateral x 50 polar angles (-45 + 5.625 k): coplanar quads, thin triangles at the interaural poles, a
    gap at the bottom"""
    lat, pol = np.meshgrid(np.radians(np.array(CIPIC_LATERAL, np.float64)), np.radians(-45.0 + 5.625 * np.arange(50)), indexing="ij")
    x, y, z = np.sin(lat), np.cos(lat) * np.cos(pol), np.cos(lat) * np.sin(pol)      # right, front, up
    azi = np.mod(np.degrees(np.arctan2(x, y)), 360.0).ravel()
    ele = np.degrees(np.arcsin(z)).ravel()
    azi32 = azi.astype(np.float32)
    azi32[azi32 >= 360.0] = 0.0
    return azi32, ele.astype(np.float32)


def kemar710():
    """the reference's own ring set through the cloud door: a gap below -40"""
    p = np.load(os.path.join(GOLD, "kemar_positions_710x2_i16.npy"))
    return p[:, 1].astype(np.float32), p[:, 0].astype(np.float32)


CLOUDS = {"fib440": fib440, "latlong410": latlong410, "cipic1250": cipic1250, "kemar710": kemar710}


def test_positions(name, n_random=20000, seed=5):
    """(ele, azi) float32: seeded uniform random directions, the lattice of every 5th whole degree, every vertex, both poles"""
    azi_v, ele_v = CLOUDS[name]()
    rng = np.random.default_rng(seed + len(azi_v))
    ele_r = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n_random)))
    azi_r = rng.uniform(0.0, 360.0, n_random)
    le, la = np.meshgrid(np.arange(-90.0, 91.0, 5.0), np.arange(0.0, 360.0, 5.0), indexing="ij")
    ele = np.concatenate([ele_r, le.ravel(), ele_v, [-90.0, 90.0]]).astype(np.float32)
    azi = np.concatenate([azi_r, la.ravel(), azi_v, [0.0, 0.0]]).astype(np.float32)
    return ele, azi
