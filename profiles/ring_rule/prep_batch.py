"""batch calls with per-kernel profiling on (prep_kernel is launched in every run), fractional positions so that the rule runs"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf
GOLD = os.path.join(ROOT, "tests", "golden")
kemar = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
sig = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")) / 8388608.0).astype(np.float32)
rng = np.random.default_rng(7)
S, K = 512, 256
e = jf.Engine(128, 512, S, hrir=kemar, max_batch_blocks=K)
for s in range(S):
    e.set_signal(s, np.roll(sig, 911 * s)[:3000])
ele = rng.uniform(-39.0, 89.0, (K, S)).astype(np.float32)
azi = rng.uniform(0.0, 360.0, (K, S)).astype(np.float32)
pos = jf.positions_from_spherical(ele, azi, np.full((K, S), 1.0, np.float32))
pos[..., 0], pos[..., 1] = ele, azi
e.profile_enable(2)
e.upload_positions(pos)
for i in range(30):
    e.batch_run(0, K)
    e.synchronize()
print(";".join(e.last_kernels()), "items", S * K)
e.close()
