// jf_room.hip -- the room stage (include/jefferson.h: jf_room_set_ir): an auxiliary send per output bus.
//
//   room_send_kernel   send_b[k] = sum over the bus's sending sources of l_s x_s, the samples the spatialiser's window takes
//                      in as new in block k (item_gather's rule, jf_kernels.hip), the level ramped over the call's first block
//   room_fft_kernel    packed spectrum of [previous send block | send block] into the bus's delay line (rv_fill_pair,
//                      rv_rfft_packed: the transform rv_forward calls)
//   room_mac_kernel    Y_ear = sum_p X[k - p] H_ear[p] for both ears from one read of the delay line (rv_load_bins; the
//                      product is this kernel's own text), the inverse transform (rv_sum_partials, rv_irfft_packed: the calls
//                      mac_finish makes), the last B samples: the wet block, interleaved
//   room_add_kernel    mix += wet
//
// DETERMINISM: the wet part is the same bits however a run is cut into calls.  No atomics; every sum has ONE
// association, fixed by the list of senders (send) or by P (products), never by the call's size K -- a (bus, block) is one
// workgroup in every kernel, and what that workgroup does depends on K nowhere but in where it finds the previous block.
//
// The transforms, their twiddles, the packing of a real spectrum (bin 0 holds the two real bins 0 and B), its split and its
// untangling are the reverb's: not copies of them but the same functions (jf_rv_small.h, the packed-spectrum toolkit); the
// responses' spectra are built by the reverb's own kernel (launch_reverb_ir, once per ear).
#include <hip/hip_runtime.h>

#include "jf_room.h"
#include "jf_packed.h"

namespace jf {

#include "jf_rv_small.h"

namespace {

typedef float __attribute__((address_space(1))) gfloat;  // float in global memory (a pointer out of a record is generic)
struct __attribute__((packed, aligned(4))) Quad4 {        // four samples at ANY sample offset: one 16-byte load
    float x, y, z, w;
};
typedef Quad4 __attribute__((address_space(1))) gquad4;

constexpr int kSendThreads = 256;

// ------------------------------------------------------------------------------------------------------ send --
// One workgroup per (block k, bus b).  A thread owns four consecutive samples of one ROW; row r takes the bus's senders
// j = r, r + ROWS, ... in ascending order, and the rows are added in ascending order out of LDS: the association depends on
// the list alone.
template <int B>
__global__ __launch_bounds__(kSendThreads) void room_send_kernel(RoomParams P) {
    constexpr int QB = B / 4, ROWS = kSendThreads / QB;
    __shared__ float4 s_part[ROWS][QB];
    const int k = blockIdx.x, b = blockIdx.y;
    const int q = threadIdx.x % QB, row = threadIdx.x / QB;
    const int j0 = P.seg[b], j1 = P.seg[b + 1];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = j0 + row; j < j1; j += ROWS) {
        const int s = P.list[j];
        const float2 lv = P.lv[j];
        const SrcSignal sg = P.sigs[s];
        const int L = sg.length;
        if (L <= 0 || sg.ptr == nullptr) continue;  // (never: a source without a signal names the engine's zeros)
        const gfloat *x = (const gfloat *)sg.ptr;
        const unsigned c0 = (unsigned)P.st_in[s].count;  // < L < 2^31, K B < 2^30: the sum fits 32 unsigned bits
        const int start = (int)((c0 + (unsigned)k * (unsigned)B) % (unsigned)L);
        float v[4];
        if (start + B <= L) {  // the block lies in one stretch of the looped signal
            const gquad4 *t = reinterpret_cast<const gquad4 *>(x + start + 4 * q);
            v[0] = t->x, v[1] = t->y, v[2] = t->z, v[3] = t->w;
        } else {  // the loop point: every sample wraps by itself
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = x[(unsigned)(start + 4 * q + c) % (unsigned)L];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            // the ramp of the call's first block: l_prev + (l_new - l_prev) (n + 1) / B -- l_new itself where they are equal
            const float l = k == 0 ? lv.x + (lv.y - lv.x) * ((float)(4 * q + c + 1) * (1.0f / (float)B)) : lv.y;
            acc[c] += l * v[c];
        }
    }
    s_part[row][q] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (row != 0) return;
    float4 t = s_part[0][q];
#pragma unroll
    for (int r = 1; r < ROWS; r++) {
        const float4 u = s_part[r][q];
        t = make_float4(t.x + u.x, t.y + u.y, t.z + u.z, t.w + u.w);
    }
    *reinterpret_cast<float4 *>(P.send + ((size_t)b * P.K + k) * B + 4 * q) = t;
    if (k == P.K - 1) *reinterpret_cast<float4 *>(P.prev_out + (size_t)b * B + 4 * q) = t;  // the next call's previous block
}

// ------------------------------------------------------------------------------------------- forward transform --
// One wavefront per (block k, bus b): the packed spectrum of x = [previous block, block] into slot head + k of the bus's
// delay line.
template <int B>
__global__ __launch_bounds__(64) void room_fft_kernel(RoomParams P) {
    __shared__ float2 s_buf[2 * B];
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float *cur = P.send + ((size_t)b * P.K + k) * B;
    const float *prv = k == 0 ? P.prev_in + (size_t)b * B : cur - B;
    rv_fill_pair<B>(s_buf, prv, cur, lane);
    // (the slot is worked out behind the transform, where the sink is called: ahead of it the division would wait for P.Rg
    // before the block's samples are asked for)
    rv_rfft_packed<B>(s_buf, s_buf + B, P.tw, lane, [&](int q, float2 x) {
        P.fdl[((size_t)b * P.Rg + (size_t)((P.head + k) % P.Rg)) * B + q] = x;
    });
}

// ---------------------------------------------------------------------------------------- multiply-accumulate --
// One workgroup of NW wavefronts per (block k, bus b).  Wave w takes the partitions p = w C .. (w + 1) C - 1, C = ceil(P /
// NW), in ascending order, a lane B / 64 consecutive bins, BOTH ears from one read of the delay line; the waves' partial
// spectra are added in ascending order of w out of LDS by the wave that then inverts the ear (wave 0 left, wave 1 right).
// A one-block call has n_buses such workgroups: a 2 s response (690 partitions at B = 128) is 44 partitions per wave, not one
// wave's chain of 690.
template <int B, int NW>
__global__ __launch_bounds__(64 * NW) void room_mac_kernel(RoomParams P) {
    constexpr int NB = B / 64, CH = 4;
    __shared__ float2 s_part[2][NW][B];
    __shared__ float2 s_fft[2][2 * B];
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool stereo = P.mono == 0;
    const int C = (P.P + NW - 1) / NW;
    const int p_lo = w * C, p_hi = min(P.P, p_lo + C);
    float2 accL[NB], accR[NB];
    float2 a0L = make_float2(0.f, 0.f), a0R = make_float2(0.f, 0.f);  // bin 0: two packed real bins, multiplied as such
#pragma unroll
    for (int i = 0; i < NB; i++) accL[i] = accR[i] = make_float2(0.f, 0.f);
    const float2 *fdl = P.fdl + (size_t)b * P.Rg * B + lane * NB;
    const float2 *hL = P.hspec + lane * NB, *hR = hL + (stereo ? P.hstride : 0);
    const int slot0 = (P.head + k) % P.Rg;  // X[k]; X[k - p] lies p slots behind it (p < P <= Rg)
#pragma unroll 1
    for (int p0 = p_lo; p0 < p_hi; p0 += CH) {
        float2 x[CH][NB], l[CH][NB], r[CH][NB];
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const int p = p0 + c < p_hi ? p0 + c : p_hi - 1;  // (past the range: loaded inside the buffers, not added)
            int sl = slot0 - p;
            sl = sl < 0 ? sl + P.Rg : sl;
            rv_load_bins<NB>(fdl + (size_t)sl * B, x[c]);
            rv_load_bins<NB>(hL + (size_t)p * B, l[c]);
            if (stereo) rv_load_bins<NB>(hR + (size_t)p * B, r[c]);
        }
#pragma unroll
        for (int c = 0; c < CH; c++) {
            if (p0 + c >= p_hi) continue;
#pragma unroll
            for (int i = 0; i < NB; i++) {
                accL[i].x += x[c][i].x * l[c][i].x - x[c][i].y * l[c][i].y;
                accL[i].y += x[c][i].x * l[c][i].y + x[c][i].y * l[c][i].x;
            }
            a0L.x += x[c][0].x * l[c][0].x;
            a0L.y += x[c][0].y * l[c][0].y;
            if (stereo) {
#pragma unroll
                for (int i = 0; i < NB; i++) {
                    accR[i].x += x[c][i].x * r[c][i].x - x[c][i].y * r[c][i].y;
                    accR[i].y += x[c][i].x * r[c][i].y + x[c][i].y * r[c][i].x;
                }
                a0R.x += x[c][0].x * r[c][0].x;
                a0R.y += x[c][0].y * r[c][0].y;
            }
        }
    }
    if (lane == 0) {
        accL[0] = a0L;
        accR[0] = a0R;
    }
#pragma unroll
    for (int i = 0; i < NB; i++) {
        s_part[0][w][lane * NB + i] = accL[i];
        s_part[1][w][lane * NB + i] = accR[i];
    }
    __syncthreads();
    const int ear = w;
    if (ear >= (stereo ? 2 : 1)) return;  // (no barrier below: the finishing waves work in LDS of their own)
    // the partial spectra in order, the packed spectrum untangled, the inverse transform: mac_finish's two calls
    rv_sum_partials<B, NW>(s_part[ear][0], B, s_fft[ear], lane);
    const float2 *zt = rv_irfft_packed<B>(s_fft[ear], s_fft[ear] + B, P.tw, lane);
    // overlap-save: time samples B .. 2B - 1 are z[m], m >= B / 2 (even, odd)
    float *wet = P.wet + ((size_t)b * P.K + k) * 2 * B;
    for (int m = B / 2 + lane; m < B; m += 64) {
        const float2 v = zt[m];
        const int n = 2 * m - B;
        if (stereo) {
            wet[2 * n + ear] = v.x;
            wet[2 * n + 2 + ear] = v.y;
        } else {
            *reinterpret_cast<float4 *>(wet + 2 * n) = make_float4(v.x, v.x, v.y, v.y);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- add --
// mix[b][k][2n + ear] = fl32(mix + wet), four floats a thread.  A wet sample that is zero leaves the mix's bits alone (a bus
// nobody ever sent to stays bit for bit what it was, the sign of a zero included).
__global__ __launch_bounds__(256) void room_add_kernel(float *__restrict__ mix, const float *__restrict__ wet, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 m = reinterpret_cast<float4 *>(mix)[i];
    const float4 v = reinterpret_cast<const float4 *>(wet)[i];
    m.x = v.x == 0.0f ? m.x : m.x + v.x;
    m.y = v.y == 0.0f ? m.y : m.y + v.y;
    m.z = v.z == 0.0f ? m.z : m.z + v.z;
    m.w = v.w == 0.0f ? m.w : m.w + v.w;
    reinterpret_cast<float4 *>(mix)[i] = m;
}

// the same for a mix that is not 16-byte aligned (jf_batch_run's d_out_mix may be any float pointer): a float a thread
__global__ __launch_bounds__(256) void room_add_scalar_kernel(float *__restrict__ mix, const float *__restrict__ wet, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = wet[i];
    if (v != 0.0f) mix[i] += v;
}

}  // namespace

// wavefronts of room_mac_kernel's workgroup (B = 256: 16 waves' partial spectra of two ears would not fit 64 KB of LDS)
constexpr int room_mac_waves_of(int B) { return B == 256 ? 8 : 16; }
int room_mac_waves(int B) { return room_mac_waves_of(B); }

// send -> forward transforms -> products and inverse: the K wet blocks of every bus, ahead of the spatialiser
hipError_t launch_room_stage(const RoomParams &P, hipStream_t st) {
    if (P.K <= 0 || P.n_buses <= 0 || P.P <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)P.K, (unsigned)P.n_buses);
    const bool known = rv_dispatch_block(P.B, [&](auto block) {
        constexpr int B = decltype(block)::value, NW = room_mac_waves_of(B);
        hipLaunchKernelGGL(room_send_kernel<B>, grid, dim3(kSendThreads), 0, st, P);
        hipLaunchKernelGGL(room_fft_kernel<B>, grid, dim3(64), 0, st, P);
        hipLaunchKernelGGL((room_mac_kernel<B, NW>), grid, dim3(64 * NW), 0, st, P);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// n floats of wet (the room's own buffer: 16-byte aligned) onto as many of mix; a mix at any float offset takes the scalar form
hipError_t launch_room_add(float *d_mix, const float *d_wet, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if ((n & 3) || ((uintptr_t)d_mix & 15) || ((uintptr_t)d_wet & 15)) {
        hipLaunchKernelGGL(room_add_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_mix, d_wet, n);
        return hipGetLastError();
    }
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(room_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, d_mix, d_wet, n4);
    return hipGetLastError();
}

}  // namespace jf
