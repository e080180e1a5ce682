// jf_ring_rule.h -- the HRTF index/weight rule of a set measured on ELEVATION RINGS (RingTable, jf_device.h), compiled for
// BOTH sides in the manner of jf_cloud_rule.h: the kernels (jf_kernels.hip) and the host (jf_host.cpp, jf_engine.cpp) include
// this one file, so jf_interpolation*, jf_grid_interpolation, jf_grid_pick, the engine's sort key and the `pick` table give
// bit for bit what the kernels compute.
//
// SoundSource.cu:65-105 and hrtf_signals.cu:20-51, float32 exactly as written.  Floor, multiply and divide only -- no libm
// call whose last bit differs between the two sides -- and no multiply-add may be contracted: every function carries the
// pragma below, whatever flags the including file is built with (a compiler without it needs -ffp-contract=off: Makefile).
//
// Domain of the picks: finite positions with |azi| < 1e6, which every caller enforces (the rules' own guards, make_desc /
// prep_body, jf_grid_pick, host_pick_hrtf); the (int)floorf(azi / inc) of the search is defined only there.
// On the host rt.pick is null or a DEVICE pointer: only ring_pick_int reads it, only the reference's rule calls that, and the
// host works that rule on ring_table() (pick = null) alone.
#pragma once
#include <math.h>

#include "jf_device.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_RING_HD __host__ __device__ __forceinline__
#else
#define JF_RING_HD inline
#endif
#if defined(__clang__)
#define JF_RING_NO_CONTRACT _Pragma("clang fp contract(off)")
#define JF_RING_UNROLL _Pragma("unroll")
#else
#define JF_RING_NO_CONTRACT
#define JF_RING_UNROLL
#endif

namespace jf {

// the nearest azimuth on a ring, the search done locally (four candidates) instead of over the whole ring
JF_RING_HD int ring_pick_azi(const RingTable &rt, int ring, float obj_azi) {
    JF_RING_NO_CONTRACT
    const float inc = rt.inc[ring];
    const int n = rt.offset[ring + 1] - rt.offset[ring];
    obj_azi = roundf(obj_azi);
    int i0 = (int)floorf(obj_azi / inc) - 1;
    if (i0 > n - 4) i0 = n - 4;
    if (i0 < 0) i0 = 0;
    float dmin = 1e37f;
    int best = 0;
    for (int i = i0; i < i0 + 4 && i < n; i++) {
        float d = obj_azi - i * inc;
        d = d > 0 ? d : -d;
        if (d < dmin) {
            dmin = d;
            best = i;
        }
    }
    return rt.offset[ring] + best;
}

// the same for an integer azimuth: one look-up in the table that search filled (jf_engine.cpp), the search itself outside it
JF_RING_HD int ring_pick_int(const RingTable &rt, int ring, int th) {
    if (rt.pick != nullptr && (unsigned)th < (unsigned)kPickAzi) return rt.pick[ring * kPickAzi + th];
    return ring_pick_azi(rt, ring, (float)th);
}

// The nearest measurement of a grid that is not the reference's (jf_engine_create_grid): the ring whose elevation is nearest
// (the lower one on a tie), on it the azimuth nearest on the circle.
JF_RING_HD int ring_grid_pick(const RingTable &rt, float ele, float azi) {
    JF_RING_NO_CONTRACT
    float dmin = 1e37f;
    int ring = 0;
    for (int r = 0; r < rt.n_rings; r++) {
        float d = ele - rt.ele[r];
        d = d > 0 ? d : -d;
        if (d < dmin) {
            dmin = d;
            ring = r;
        }
    }
    const int n = rt.offset[ring + 1] - rt.offset[ring];
    float a = azi - 360.0f * floorf(azi / 360.0f);
    if (!(a < 360.0f)) a = 0.0f;
    int i = (int)floorf(a / rt.inc[ring] + 0.5f);
    if (i >= n) i = 0;  // nearer to 360 = the ring's first entry
    return rt.offset[ring] + i;
}

// hrtf_signals.cu:20-51 in full: nearest elevation ring, then nearest azimuth on it.  The reference's grid (rt.kemar) has ring
// e at -40 + 10 e degrees, the form the reference's rule below finds its rings by; rt.ele[e] holds the same values, but read
// from the kernel's arguments they made every kernel with this code inlined slower, FD_BASIC or not (the one-launch
// kernel by 0.7 us per block: profiles/ring_rule/README.md).
JF_RING_HD int ring_pick_hrtf(const RingTable &rt, float obj_ele, float obj_azi) {
    JF_RING_NO_CONTRACT
    if (!rt.kemar) return ring_grid_pick(rt, obj_ele, obj_azi);
    obj_ele = roundf(obj_ele / 10) * 10;
    float dmin = 1e37f;
    int ring = 0;
    for (int e = 0; e < kNumElev; e++) {
        float d = obj_ele - (float)(-40 + 10 * e);
        d = d > 0 ? d : -d;
        if (d < dmin) {
            dmin = d;
            ring = e;
        }
    }
    return ring_pick_azi(rt, ring, obj_azi);
}

// SoundSource.cu:65-105, the reference's rule on the reference's grid (rt.kemar): table rows h[4], weights om[6] = omegaA ..
// omegaF.  false: no answer (silence).
// (-50, 91): where both truncated elevations name a measured ring.  The setters' whole degrees end at 90; a latched record
// may carry 90.x, which the reference's statements place on the 90-degree ring twice (weights 0.x and -0.x)
JF_RING_HD bool ring_interp_reference(const RingTable &rt, float ele, float azi, int h[4], float om[6]) {
    JF_RING_NO_CONTRACT
    if (!(ele > -50.0f && ele < 91.0f) || !(azi > -1.0e6f && azi < 1.0e6f)) return false;
    const int phi0 = (int)(ele) / 10 * 10;
    const int phi1 = (int)(ele + 9) / 10 * 10;
    // the rings with these elevations (multiples of 10 by construction; -40 .. 90 exist: ring r at -40 + 10 r)
    const int r0 = (phi0 >= -40 && phi0 <= 90) ? (phi0 + 40) / 10 : -1;
    const int r1 = (phi1 >= -40 && phi1 <= 90) ? (phi1 + 40) / 10 : -1;
    if (r0 < 0 || r1 < 0) return false;
    const float dt1 = rt.inc[r0], dt2 = rt.inc[r1];
    const int th0 = (int)((int)(azi / dt1) * dt1);
    const int th1 = (int)((int)((azi + dt1 - 1) / dt1) * dt1);
    const int th2 = (int)((int)(azi / dt2) * dt2);
    const int th3 = (int)((int)((azi + dt2 - 1) / dt2) * dt2);
    om[0] = (azi - th0) / dt1;
    om[1] = (th1 - azi) / dt1;
    om[2] = (azi - th2) / dt2;
    om[3] = (th3 - azi) / dt2;
    om[4] = (ele - phi0) / 10.0f;
    om[5] = (phi1 - ele) / 10.0f;
    h[0] = ring_pick_int(rt, r0, th0);
    h[1] = ring_pick_int(rt, r0, th1);
    h[2] = ring_pick_int(rt, r1, th2);
    h[3] = ring_pick_int(rt, r1, th3);
    return true;
}

// The corrected rule behind JF_FLAG_CORRECTED_INTERPOLATION (not in the reference):
// true floor of the elevation, azimuth folded into [0, 360) with a ring's last interval wrapping to its first
// entry, float azimuths (a ring's two weights sum to 1), elevations below the lowest ring clamped to it.
// Same index order and weight meaning as the reference's rule.  Float32 step by step as in the oracles.
// In its general form (any grid of rings, include/jefferson.h: jf_hrtf_grid): the ring pair is the one whose elevations
// enclose the position (elevations outside the grid clamped to its first / last ring), the elevation weight is linear between
// them.  For the reference's grid the closed form below gives the same ring, the same phi0 and the same divisor 10 -- bit for
// bit the same indices and weights (tests/test_abi.py compares the two on the host, tests/test_gpu_grid.py on the GPU).
JF_RING_HD bool ring_interp_corrected(const RingTable &rt, float ele, float azi, int h[4], float om[6]) {
    JF_RING_NO_CONTRACT
    if (!(ele <= 90.0f) || !(ele > -1.0e6f) || !(azi > -1.0e6f && azi < 1.0e6f)) return false;
    float a = azi - 360.0f * floorf(azi / 360.0f);
    if (!(a < 360.0f)) a = 0.0f;
    int r0;
    float phi0, span;
    if (rt.kemar) {
        if (ele < -40.0f) ele = -40.0f;
        const float q = floorf(ele / 10.0f);
        phi0 = 10.0f * q;
        r0 = (int)q + 4;
        span = 10.0f;
    } else {
        const int last = rt.n_rings - 1;
        if (ele < rt.ele[0]) ele = rt.ele[0];
        if (ele > rt.ele[last]) ele = rt.ele[last];
        r0 = 0;
        for (int r = 1; r <= last; r++) r0 = rt.ele[r] <= ele ? r : r0;
        phi0 = rt.ele[r0];
        span = rt.ele[r0 < last ? r0 + 1 : r0] - phi0;
    }
    const bool on_ring = ele == phi0;
    const float omE = on_ring ? 0.0f : (ele - phi0) / span;
    const int ring[2] = {r0, on_ring ? r0 : r0 + 1};
    JF_RING_UNROLL
    for (int j = 0; j < 2; j++) {  // the ring's two entries around the folded azimuth and their weights
        const int r = ring[j];
        const float d = rt.inc[r];
        const int n = rt.offset[r + 1] - rt.offset[r];
        int i0 = (int)floorf(a / d);
        if (i0 > n - 1) i0 = n - 1;
        float wa = (a - (float)i0 * d) / d;
        if (wa < 0.0f) wa = 0.0f;
        if (wa > 1.0f) wa = 1.0f;
        if (n == 1) wa = 0.0f;
        int i1 = i0 + 1 == n ? 0 : i0 + 1;
        if (wa == 0.0f) i1 = i0;
        h[2 * j] = rt.offset[r] + i0;
        h[2 * j + 1] = rt.offset[r] + i1;
        om[2 * j] = wa;
        om[2 * j + 1] = 1.0f - wa;
    }
    om[4] = omE;
    om[5] = 1.0f - omE;
    return true;
}

// GPUSoundSource.cu:301-316: the case by index equality, flattened to <= 4 (row, weight) terms; returns their number (1, 2
// or 4).  Written with selects, not branches: the compiler merges the branches' stores `w[i] = ..` into one store at a
// run-time index, which puts the arrays into scratch memory (24 bytes that every kernel with this code inlined then
// carries).  The same values: the four products are formed whether or not case 4 uses them.
JF_RING_HD int ring_flatten_terms(int h0, int h1, int h2, int h3, float omegaA, float omegaB, float omegaC, float omegaD,
                                  float omegaE, float omegaF, int rows[4], float w[4]) {
    JF_RING_NO_CONTRACT
    const bool c1 = h0 == h1 && h1 == h2 && h2 == h3;    // one row
    const bool c2 = !c1 && h0 == h2 && h1 == h3;          // elevation on a ring: two azimuths
    const bool c3 = !c1 && !c2 && h0 == h1 && h0 != h2;   // azimuth on the grid: two rings
    const bool c4 = !c1 && !c2 && !c3;
    const float fb = omegaF * omegaB, fa = omegaF * omegaA, ed = omegaE * omegaD, ec = omegaE * omegaC;
    rows[0] = h0;
    w[0] = c1 ? 1.0f : c2 ? omegaB : c3 ? omegaF : fb;
    rows[1] = c1 ? h0 : c3 ? h2 : h1;
    w[1] = c1 ? 0.0f : c2 ? omegaA : c3 ? omegaE : fa;
    rows[2] = c4 ? h2 : h0;
    w[2] = c4 ? ed : 0.0f;
    rows[3] = c4 ? h3 : h0;
    w[3] = c4 ? ec : 0.0f;
    return c1 ? 1 : c4 ? 4 : 2;
}

}  // namespace jf
