// jf_output_rule.h -- the BUS OUTPUT rule (include/jefferson.h: "bus outputs"): a rational polyphase resampler
// from the engine's 44 100 Hz to a codec's rate, the mirror image of jf_stream_rule.h.  Compiled for BOTH sides in the manner of
// that file: the kernel (jf_output.hip) and the host twin (jf_output_resample, which the CPU suite checks bit for bit against a
// NumPy model) include this one file and get the same bits.  Self-contained: a plain C++ compiler can build it.  Nothing here
// calls libm on the device: the table is built on the host in double (output_table_build, host only) and the device reads it.
//
// RATES.  g = gcd(R, 44100), L = R / g phases, M = 44100 / g.  Accepted: 8000 <= R <= 48000 with L <= 480 and M <= 441 (every
// multiple of 100 Hz in range, and 11 025 and 22 050: the rates a stream source takes, jf_stream_rule.h with L and M changing
// places).  R == 44100 (L = M = 1) is a pure FIFO: no filter, no delay (T = 1, D = 0).
// INDEXING.  Output frame u (a 64-bit count since the output was set or reset) stands at input frame i(u) = floor(u M / L) with
// phase p(u) = u M mod L.  The first N input frames determine produced(N) = ceil(N L / M) outputs: exactly those u with
// i(u) <= N - 1.  A call that renders n frames after N0 yields produced(N0 + n) - produced(N0) outputs.
// TAPS.  T = 64 s taps, s the smallest power of two with s L >= M (1 at 48 000 Hz, 8 at 8 000 Hz: T <= 512), a delay of
// D = T / 2 - 1 input frames.  Per channel  y[u] = sum_{k < T} h[p][k] x[i - k],  x[j] = 0 for j < 0,
//   h[p][k] = c sinc(c tau) w(tau),  tau = k - D + p / L,  c = 0.94 min(1, L / M),  w(tau) = I0(9 sqrt(1 - (tau / (T/2 + 1))^2)) / I0(9),
// every row normalised in double to sum 1 and then rounded once to float32.
// ACCUMULATION, the same on both sides and for both ears (one row serves left and right): four float32 accumulators a_j = +0;
// tap k goes into a_{k mod 4} in ascending k, each term a float32 product rounded and a float32 add rounded (contraction off);
// the result is (a0 + a1) + (a2 + a3).
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_OUTPUT_HD __host__ __device__ __forceinline__
#else
#define JF_OUTPUT_HD inline
#endif
#if defined(__clang__)
#define JF_OUTPUT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_OUTPUT_NO_CONTRACT
#endif

namespace jf {

constexpr int kOutputInRate = 44100;  // the engine's rate (main.cu:79, main.cu:93)
constexpr int kOutputMaxL = 480;
constexpr int kOutputMaxM = 441;
constexpr int kOutputMinRate = 8000, kOutputMaxRate = 48000;
constexpr int kOutputMaxTaps = 512;   // T at 8 000 Hz
constexpr int kOutputHist = kOutputMaxTaps - 1;  // input frames behind a call's first that its outputs may read
constexpr int kOutputTile = 256;      // output frames a workgroup of the kernel forms
// Input frames a tile of kOutputTile outputs reads at most.  Its first and last output stand floor((p + 255 M) / L) frames apart,
// p <= L - 1: at most floor(255 M / L + (L - 1) / L).  M / L is largest at 8000 Hz (441 / 80, T = 512): floor(1405.7 + 0.99) =
// 1406, so 1407 positions, and the first reaches T - 1 = 511 frames back.  Every other rate spans less: the rates with T = 512
// (below 11 025 Hz) have 255 M / L <= 255 * 441 / 81 = 1388.4, the others at most 255 * 4 + 1 positions and 255 frames back.
constexpr int kOutputSpanMax = 1407 + kOutputHist;  // 1918 stereo frames: 15 344 bytes of LDS

// L, M and T of a rate; false: the rate is not accepted
JF_OUTPUT_HD bool output_ratio(int rate, int *L, int *M, int *T) {
    if (rate < kOutputMinRate || rate > kOutputMaxRate) return false;
    int a = rate, b = kOutputInRate;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    const int l = rate / a, m = kOutputInRate / a;
    if (l > kOutputMaxL || m > kOutputMaxM) return false;
    int s = 1;
    while (s * l < m) s *= 2;
    *L = l;
    *M = m;
    *T = rate == kOutputInRate ? 1 : 64 * s;
    return true;
}

// i(u) and p(u) for u >= 0 (u M < 2^63 for every u up to 2^53), produced(N) for N >= 0 (N L likewise)
JF_OUTPUT_HD long long output_index(long long u, int L, int M) { return (u * (long long)M) / L; }
JF_OUTPUT_HD int output_phase(long long u, int L, int M) { return (int)((u * (long long)M) % L); }
JF_OUTPUT_HD long long output_produced(long long N, int L, int M) { return (N * (long long)L + M - 1) / M; }

// The accumulators of one output frame, both ears.
struct OutputAcc {
    float l0, l1, l2, l3, r0, r1, r2, r3;
};
JF_OUTPUT_HD OutputAcc output_acc_zero() { return OutputAcc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
// Taps k .. k + 3 (k a multiple of 4): h0 .. h3 the row's entries, (xl_j, xr_j) the frame x[i - k - j].
JF_OUTPUT_HD void output_acc4(OutputAcc &a, float h0, float h1, float h2, float h3, float xl0, float xr0, float xl1, float xr1,
                              float xl2, float xr2, float xl3, float xr3) {
    JF_OUTPUT_NO_CONTRACT
    const float ml0 = h0 * xl0, mr0 = h0 * xr0;
    const float ml1 = h1 * xl1, mr1 = h1 * xr1;
    const float ml2 = h2 * xl2, mr2 = h2 * xr2;
    const float ml3 = h3 * xl3, mr3 = h3 * xr3;
    a.l0 = a.l0 + ml0;
    a.r0 = a.r0 + mr0;
    a.l1 = a.l1 + ml1;
    a.r1 = a.r1 + mr1;
    a.l2 = a.l2 + ml2;
    a.r2 = a.r2 + mr2;
    a.l3 = a.l3 + ml3;
    a.r3 = a.r3 + mr3;
}
JF_OUTPUT_HD void output_acc_sum(const OutputAcc &a, float *l, float *r) {
    JF_OUTPUT_NO_CONTRACT
    *l = (a.l0 + a.l1) + (a.l2 + a.l3);
    *r = (a.r0 + a.r1) + (a.r2 + a.r3);
}

// One output frame from its T taps (T a multiple of 4): h = the phase's row, x = a pointer to the interleaved frame x[i] with
// the frames x[i - 1] .. x[i - T + 1] valid behind it.
JF_OUTPUT_HD void output_dot(const float *h, const float *x, int T, float *l, float *r) {
    OutputAcc a = output_acc_zero();
    for (int k = 0; k < T; k += 4) {
        const float *f = x - 2 * k;
        output_acc4(a, h[k], h[k + 1], h[k + 2], h[k + 3], f[0], f[1], f[-2], f[-1], f[-4], f[-3], f[-6], f[-5]);
    }
    output_acc_sum(a, l, r);
}

}  // namespace jf
