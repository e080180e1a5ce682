// jf_kernels2048.hip -- the PAD_LEN 2048 path (gfx950): configurations whose B + hrtf_len - 1 pads to 2048
// (Universal.cuh:9-12 with HRTF_LEN up to 2049 - B), Nc = 1025 bins.  Same work as the PAD_LEN 1024 kernels of
// jf_kernels.hip, in the same order and with the same operand order (GPUSoundSource.cu:320-385, :463-513), by a
// WORKGROUP per unit instead of a wave: a 2048-point complex transform is 16 KB of LDS and 32 values per lane of one
// wave -- past what a wave can keep in registers at the headline kernel's occupancy.
//
// Table (engine-owned, built by table2048_build_kernel):
//   htab  float4[n_rows][1024]  k >= 1: {L.re, L.im, R.re, R.im};  k == 0: {L[0].re, L[1024].re, R[0].re, R[1024].re}
//                               -- the layout of the 1024 table (jf_device.h) at twice the length: one 16-byte load per
//                               bin fetches both ears, a row is 16 KiB.
//
// fused2048_kernel: one workgroup of 256 threads per unit = (block b, G consecutive sources):
//   per PAIR of sources: both windows as one complex signal x_a + i x_b -> one forward 2048-point transform (LDS
//     Stockham, radix 4^5 x 2) -> X_a, X_b from Z[k] and Z[N-k];
//   per source: X D (distance factor by the exact phase word of distance_from_phase, divisor Nc = 1025), times
//     sum_t w_t H[row_t] for both ears, ADDED to the unit's spectral sums of the new and (if any source of the unit
//     cross-fades) the old filter set: a source that did not move carries its new set into both sums;
//   per unit: Z = Y_L + i Y_R of each set -> one inverse 2048-point transform per set (both ears at once) -> the last
//     B outputs, cross-faded (f = n / (B - 1), kernels.cu:132-137), stored as the unit's partial stereo block for
//     mix_kernel / mix_few_kernel.
// Thread t keeps bins k = t + 256 j, j = 0..3, of every sum; thread 0 keeps bin 1024 in the imaginary slot of bin 0
// (bins 0 and N/2 of a real signal are real, and a c2r ignores their imaginary parts).
#include <hip/hip_runtime.h>

#include "jf_device.h"
#include "jf_phase.h"

namespace jf {

namespace {

#define JF_DEV2 __device__ __forceinline__

constexpr int kN2 = 2048;
constexpr int kT2 = 256;  // threads per workgroup
constexpr int kBins2 = kN2 / 2 / kT2;  // 4 bins per thread (plus bin 1024 on thread 0)

JF_DEV2 float2 c_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
JF_DEV2 float2 c_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
JF_DEV2 float2 c_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a * w (DIR = +1) or a * conj(w) (DIR = -1); w from the table exp(+2 pi i j / 2048)
template <int DIR>
JF_DEV2 float2 c_tw(float2 a, float2 w) {
    return DIR > 0 ? c_mul(a, w) : make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y);
}
// a * (-i) for the forward transform, a * (+i) for the inverse
template <int DIR>
JF_DEV2 float2 c_rot(float2 a) {
    return DIR > 0 ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
}

// In-place 2048-point complex DFT of buf (natural order in and out), unnormalised, exp(DIR 2 pi i jk / N), by the
// 256 threads of the workgroup: Stockham passes radix 4, 4, 4, 4, 4, 2.  Each pass reads all its inputs into registers,
// meets the workgroup at a barrier, writes its outputs to the same buffer and meets it again.  tw: exp(+2 pi i j / 2048)
// in LDS.  The caller has put the input in buf and passed a barrier.
template <int DIR>
JF_DEV2 void fft2048(float2 *buf, const float2 *tw, int tid) {
#pragma unroll
    for (int pass = 0; pass < 5; pass++) {
        const int ls = 2 * pass;  // Ns = 4^pass
        const int Ns = 1 << ls;
        float2 v[2][4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = tid + kT2 * h;  // butterfly 0 .. 511
            const int jm = j & (Ns - 1);
            const int step = jm << (9 - ls);  // jm N / (4 Ns): twiddle exponent of input r is r step (< 1536)
#pragma unroll
            for (int r = 0; r < 4; r++) v[h][r] = buf[j + 512 * r];
#pragma unroll
            for (int r = 1; r < 4; r++) v[h][r] = c_tw<DIR>(v[h][r], tw[r * step]);
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = tid + kT2 * h;
            const int jm = j & (Ns - 1);
            const float2 a0 = c_add(v[h][0], v[h][2]), a1 = c_sub(v[h][0], v[h][2]);
            const float2 a2 = c_add(v[h][1], v[h][3]), a3 = c_rot<DIR>(c_sub(v[h][1], v[h][3]));
            const int o = ((j >> ls) << (ls + 2)) + jm;
            buf[o] = c_add(a0, a2);
            buf[o + Ns] = c_add(a1, a3);
            buf[o + 2 * Ns] = c_sub(a0, a2);
            buf[o + 3 * Ns] = c_sub(a1, a3);
        }
        __syncthreads();
    }
    // radix 2, Ns = 1024: butterfly j pairs j and j + 1024, twiddle exponent j
    float2 v[4][2];
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const int j = tid + kT2 * h;
        v[h][0] = buf[j];
        v[h][1] = c_tw<DIR>(buf[j + 1024], tw[j]);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const int j = tid + kT2 * h;
        buf[j] = c_add(v[h][0], v[h][1]);
        buf[j + 1024] = c_sub(v[h][0], v[h][1]);
    }
    __syncthreads();
}

// Two real signals a, b transformed together as z = a + i b: 2 A[k] = Z[k] + conj Z[N-k], 2 B[k] = -i (Z[k] - conj Z[N-k]).
// One of them (second: b) out of the transform in buf.  Bins k = tid + 256 j; on thread 0 slot 0 is (2 A[0], 2 A[1024])
// (or (2 B[0], 2 B[1024])).  TWICE the spectrum.
JF_DEV2 void split_one(const float2 *buf, int tid, bool second, float2 (&x)[kBins2]) {
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        const int k = tid + kT2 * j;
        const float2 zk = buf[k], zm = buf[(kN2 - k) & (kN2 - 1)];
        x[j] = second ? make_float2(zk.y + zm.y, zm.x - zk.x) : make_float2(zk.x + zm.x, zk.y - zm.y);
    }
    if (tid == 0) {
        const float2 z0 = buf[0], zh = buf[kN2 / 2];
        x[0] = second ? make_float2(2.0f * z0.y, 2.0f * zh.y) : make_float2(2.0f * z0.x, 2.0f * zh.x);
    }
}

// One source's window for block b: window sample n = tid + 256 m has q = b B + n - (N - B); q < 0 from the previous
// call's window, else the looped signal (every device signal has length >= 2048: jf_source_set_signal).
JF_DEV2 void gather2048(const FusedParams &P, int b, int s, int tid, float (&x)[8], int &count0, int &L) {
    const SrcSignal sg = P.sigs[s];
    count0 = P.st_in[s].count;
    L = sg.length;
    const float *hist = P.hist_in + (size_t)s * kN2;
    const int q0 = b * P.B - (kN2 - P.B);
    const int qpos = q0 > 0 ? q0 : 0;
    const int base = (int)(((long long)count0 + qpos) % L) - qpos;  // signal index of q = 0 (mod L)
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int q = q0 + tid + kT2 * m;
        if (q < 0) {
            x[m] = hist[kN2 + q];
        } else {
            int idx = base + q;  // in [0, L + N)
            idx = idx >= L ? idx - L : idx;
            x[m] = sg.ptr[idx];
        }
    }
}

// last block of the call: leave the window and the counters for the next call
JF_DEV2 void write_back2048(const FusedParams &P, int s, int tid, const float (&x)[8], int count0, int L) {
    float *ho = P.hist_out + (size_t)s * kN2;
#pragma unroll
    for (int m = 0; m < 8; m++) ho[tid + kT2 * m] = x[m];
    if (tid == 0) {
        SrcState st;
        st.count = (int)(((long long)count0 + (long long)P.K * P.B) % L);
        const float *pp = P.pos + ((size_t)(P.K - 1) * P.S + s) * 5;
        st.old_ele = pp[0];
        st.old_azi = pp[1];
        st.pad = 0;
        P.st_out[s] = st;
    }
}

// he = sum_t w_t H[row_t][k] (both ears in one float4): a multiply by the first weight, then one FMA per further row
JF_DEV2 void weighted_rows(const float4 *htab, const int *rows, const float *w, int n, int tid, float4 (&he)[kBins2]) {
    const float4 *h0 = htab + (size_t)rows[0] * (kN2 / 2) + tid;
    const float w0 = w[0];
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        const float4 h = h0[kT2 * j];
        he[j] = make_float4(w0 * h.x, w0 * h.y, w0 * h.z, w0 * h.w);
    }
    for (int t = 1; t < n; t++) {
        const float4 *ht = htab + (size_t)rows[t] * (kN2 / 2) + tid;
        const float wt = w[t];
#pragma unroll
        for (int j = 0; j < kBins2; j++) {
            const float4 h = ht[kT2 * j];
            he[j] = make_float4(fmaf(wt, h.x, he[j].x), fmaf(wt, h.y, he[j].y), fmaf(wt, h.z, he[j].z),
                                fmaf(wt, h.w, he[j].w));
        }
    }
}

// y_ear[j] += xd[j] * he_ear[j]; slot 0 of thread 0 holds two real bins (0 and 1024): element-wise products there
JF_DEV2 void add_products(const float2 (&xd)[kBins2], const float4 (&he)[kBins2], int tid, float2 (&yl)[kBins2],
                          float2 (&yr)[kBins2]) {
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        const float2 hl = make_float2(he[j].x, he[j].y), hr = make_float2(he[j].z, he[j].w);
        if (j == 0 && tid == 0) {
            yl[0] = make_float2(yl[0].x + xd[0].x * hl.x, yl[0].y + xd[0].y * hl.y);
            yr[0] = make_float2(yr[0].x + xd[0].x * hr.x, yr[0].y + xd[0].y * hr.y);
        } else {
            yl[j] = c_add(yl[j], c_mul(xd[j], hl));
            yr[j] = c_add(yr[j], c_mul(xd[j], hr));
        }
    }
}

// One source's contribution to the unit's sums.  x: twice its spectrum (split_pair); the 1/N of the forward transform
// and the 1/2 of the split ride on 1/frac (powers of two: exact).
JF_DEV2 void accumulate_source(const FusedParams &P, const ItemDesc *dp, const float2 (&x)[kBins2], bool xf, int tid,
                               float2 (&yn)[2][kBins2], float2 (&yo)[2][kBins2]) {
    const unsigned long long c64 = dp->c_fix;
    const float sinv = dp->inv_frac * (1.0f / (2.0f * kN2));
    float2 xd[kBins2];
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        const unsigned long long k = (unsigned long long)(tid + kT2 * j);
        xd[j] = c_mul(x[j], distance_from_phase((unsigned)((k * c64) >> 32), sinv));
    }
    if (tid == 0) {
        const float d1024 = distance_from_phase((unsigned)((c64 << 10) >> 32), sinv).x;
        xd[0] = make_float2(x[0].x * sinv, x[0].y * d1024);
    }
    float4 he[kBins2];
    weighted_rows(P.htab, dp->rows_new, dp->w_new, dp->n_new, tid, he);
    add_products(xd, he, tid, yn[0], yn[1]);
    if (xf) {
        if (dp->n_old > 0) weighted_rows(P.htab, dp->rows_old, dp->w_old, dp->n_old, tid, he);
        add_products(xd, he, tid, yo[0], yo[1]);
    }
}

// Z = Y_L + i Y_R over all 2048 bins (Z[N-k] = conj Y_L[k] + i conj Y_R[k]) into buf, then the inverse transform
JF_DEV2 void inverse_set(float2 *buf, const float2 *tw, int tid, const float2 (&yl)[kBins2], const float2 (&yr)[kBins2]) {
    __syncthreads();  // every reader of buf is done
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        const int k = tid + kT2 * j;
        if (j == 0 && tid == 0) {
            buf[0] = make_float2(yl[0].x, yr[0].x);
            buf[kN2 / 2] = make_float2(yl[0].y, yr[0].y);
        } else {
            buf[k] = make_float2(yl[j].x - yr[j].y, yl[j].y + yr[j].x);
            buf[kN2 - k] = make_float2(yl[j].x + yr[j].y, yr[j].x - yl[j].y);
        }
    }
    __syncthreads();
    fft2048<1>(buf, tw, tid);
}

}  // namespace

__global__ __launch_bounds__(kT2) void fused2048_kernel(const FusedParams P) {
    __shared__ float2 s_tw[kN2];
    __shared__ float2 s_buf[kN2];
    const int tid = threadIdx.x;
    for (int j = tid; j < kN2; j += kT2) s_tw[j] = P.tw[j];  // (a barrier comes before the first transform)
    const int G = P.G, SG = P.S / G, B = P.B;
    // consecutive workgroups take consecutive blocks of the same sources: their table rows and windows overlap in cache
    const int sg = (int)blockIdx.x / P.K;
    const int b = (int)blockIdx.x - sg * P.K;
    const int s0 = sg * G;
    const ItemDesc *desc = P.desc + (size_t)b * P.S + s0;
    // the unit cross-fades if any of its sounding sources does (then every sounding source adds to both sums)
    bool xf = false, any = false;
    for (int g = 0; g < G; g++) {
        const bool on = desc[g].n_new > 0;
        any = any || on;
        xf = xf || (on && desc[g].n_old > 0);
    }
    float2 yn[2][kBins2], yo[2][kBins2];
#pragma unroll
    for (int j = 0; j < kBins2; j++) yn[0][j] = yn[1][j] = yo[0][j] = yo[1][j] = make_float2(0.f, 0.f);
#pragma unroll 1
    for (int g = 0; g < G; g += 2) {
        const bool pair = g + 1 < G;
        float xa[8], xb[8];
        int ca, la, cb = 0, lb = 1;
        gather2048(P, b, s0 + g, tid, xa, ca, la);
        if (pair) {
            gather2048(P, b, s0 + g + 1, tid, xb, cb, lb);
        } else {
#pragma unroll
            for (int m = 0; m < 8; m++) xb[m] = 0.0f;
        }
        if (b == P.K - 1) {
            write_back2048(P, s0 + g, tid, xa, ca, la);
            if (pair) write_back2048(P, s0 + g + 1, tid, xb, cb, lb);
        }
        const bool on_a = desc[g].n_new > 0, on_b = pair && desc[g + 1].n_new > 0;
        if (!on_a && !on_b) continue;  // (workgroup-uniform) silent: not interpolable, no defined output
        __syncthreads();  // the previous pair's reads of s_buf are done
#pragma unroll
        for (int m = 0; m < 8; m++) s_buf[tid + kT2 * m] = make_float2(xa[m], xb[m]);
        __syncthreads();
        fft2048<-1>(s_buf, s_tw, tid);
        // (s_buf holds the pair's transform until the next pair's barrier: each source's bins are read when needed)
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            if (!(h ? on_b : on_a)) continue;
            float2 X[kBins2];
            split_one(s_buf, tid, h != 0, X);
            accumulate_source(P, desc + g + h, X, xf, tid, yn, yo);
        }
    }
    float2 *out = reinterpret_cast<float2 *>(P.partial) + ((size_t)b * SG + sg) * B;
    if (!any) {
        if (tid < B) out[tid] = make_float2(0.f, 0.f);
        return;
    }
    float2 old_frame = make_float2(0.f, 0.f);
    if (xf) {
        inverse_set(s_buf, s_tw, tid, yo[0], yo[1]);
        if (tid < B) old_frame = s_buf[kN2 - B + tid];
    }
    inverse_set(s_buf, s_tw, tid, yn[0], yn[1]);
    if (tid < B) {
        float2 r = s_buf[kN2 - B + tid];
        if (xf) {
            // kernels.cu:132-137
            const float fn = (float)tid / ((float)B - 1.0f);
            r = make_float2(old_frame.x * (1.0f - fn) + r.x * fn, old_frame.y * (1.0f - fn) + r.y * fn);
        }
        out[tid] = r;
    }
}

// The table: unnormalised r2c of each [row][ear][2048] zero-padded impulse response (transform_hrtfs at PAD_LEN 2048),
// both ears of a row through one complex transform.
__global__ __launch_bounds__(kT2) void table2048_build_kernel(const float *__restrict__ hrir, int taps,
                                                             const float2 *__restrict__ twg, float4 *__restrict__ htab) {
    __shared__ float2 s_tw[kN2];
    __shared__ float2 s_buf[kN2];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    for (int j = tid; j < kN2; j += kT2) s_tw[j] = twg[j];
    const float *hl = hrir + (size_t)row * 2 * taps, *hr = hl + taps;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int n = tid + kT2 * m;
        s_buf[n] = make_float2(n < taps ? hl[n] : 0.0f, n < taps ? hr[n] : 0.0f);
    }
    __syncthreads();
    fft2048<-1>(s_buf, s_tw, tid);
    float2 XL[kBins2], XR[kBins2];
    split_one(s_buf, tid, false, XL);
    split_one(s_buf, tid, true, XR);
    float4 *o = htab + (size_t)row * (kN2 / 2) + tid;
#pragma unroll
    for (int j = 0; j < kBins2; j++) o[kT2 * j] = make_float4(0.5f * XL[j].x, 0.5f * XL[j].y, 0.5f * XR[j].x, 0.5f * XR[j].y);
}

// parity tap: unnormalised r2c spectra [n][1025] of arbitrary 2048-sample windows with the same transform
__global__ __launch_bounds__(kT2) void rfft2048_debug_kernel(const float *__restrict__ win, const float2 *__restrict__ twg,
                                                            float2 *__restrict__ spec) {
    __shared__ float2 s_tw[kN2];
    __shared__ float2 s_buf[kN2];
    const int tid = threadIdx.x;
    for (int j = tid; j < kN2; j += kT2) s_tw[j] = twg[j];
    const float *x = win + (size_t)blockIdx.x * kN2;
#pragma unroll
    for (int m = 0; m < 8; m++) s_buf[tid + kT2 * m] = make_float2(x[tid + kT2 * m], 0.0f);
    __syncthreads();
    fft2048<-1>(s_buf, s_tw, tid);
    float2 X[kBins2];
    split_one(s_buf, tid, false, X);
    float2 *o = spec + (size_t)blockIdx.x * (kN2 / 2 + 1);
#pragma unroll
    for (int j = 0; j < kBins2; j++) {
        if (j == 0 && tid == 0) {
            o[0] = make_float2(0.5f * X[0].x, 0.0f);
            o[kN2 / 2] = make_float2(0.5f * X[0].y, 0.0f);
        } else {
            o[tid + kT2 * j] = make_float2(0.5f * X[j].x, 0.5f * X[j].y);
        }
    }
}

hipError_t launch_fused2048(const FusedParams &P, hipStream_t st) {
    if (P.G <= 0 || P.S % P.G != 0 || P.B > kT2 || P.B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fused2048_kernel, dim3(P.K * (P.S / P.G)), dim3(kT2), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_table2048_build(const float *d_hrir, int n_rows, int taps, const float2 *d_tw2048, float4 *d_htab,
                                  hipStream_t st) {
    if (taps <= 0 || taps > kN2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(table2048_build_kernel, dim3(n_rows), dim3(kT2), 0, st, d_hrir, taps, d_tw2048, d_htab);
    return hipGetLastError();
}

hipError_t launch_rfft2048_debug(const float *d_win, int n, const float2 *d_tw2048, float2 *d_spec, hipStream_t st) {
    hipLaunchKernelGGL(rfft2048_debug_kernel, dim3(n), dim3(kT2), 0, st, d_win, d_tw2048, d_spec);
    return hipGetLastError();
}

}  // namespace jf
