// jf_stream_rule.h -- the STREAM SOURCE rule (include/jefferson.h: "stream sources"): a rational polyphase
// resampler from a codec's rate to the engine's 44 100 Hz.  Compiled for BOTH sides in the manner of jf_gate_rule.h: the kernel
// (jf_stream.hip) and the host twin (jf_stream_resample, which the CPU suite checks bit for bit against a NumPy model) include
// this one file and get the same bits.  Self-contained: a plain C++ compiler can build it.  Nothing here calls libm on the
// device: the table is built on the host in double (stream_table_build, host only) and the device reads it.
//
// RATES.  g = gcd(rate, 44100), L = 44100 / g phases, M = rate / g.  Accepted: 8000 <= rate <= 48000 with L <= 441 (every
// multiple of 100 Hz in range, and 11 025 and 22 050).  rate == 44100 (L = M = 1) is a pure FIFO: no filter, no delay.
// INDEXING.  Output sample t (a 64-bit count since the stream started) stands at input i(t) = floor(t M / L) with phase
// p(t) = t M mod L; i(-1) := -1.  A call of n outputs from t0 needs need(t0, n) = i(t0 + n - 1) - i(t0 - 1) new frames.
// TAPS.  T = 64 taps, a delay of D = 31 input frames:  y[t] = sum_{k < 64} h[p][k] x[i - k],  x[j] = 0 for j < 0,
//   h[p][k] = c sinc(c tau) w(tau),  tau = k - D + p / L,  c = 0.94 min(1, L / M),  w(tau) = I0(9 sqrt(1 - (tau / 33)^2)) / I0(9),
// every row normalised in double to sum 1 and then rounded once to float32.
// ACCUMULATION, the same on both sides: four float32 accumulators a_j = +0; tap k goes into a_{k mod 4} in ascending k, each
// term a float32 product rounded and a float32 add rounded (contraction off); the result is (a0 + a1) + (a2 + a3).
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_STREAM_HD __host__ __device__ __forceinline__
#else
#define JF_STREAM_HD inline
#endif
#if defined(__clang__)
#define JF_STREAM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_STREAM_NO_CONTRACT
#endif

namespace jf {

constexpr int kStreamOutRate = 44100;  // the engine's rate (main.cu:79, main.cu:93)
constexpr int kStreamTaps = 64;        // T
constexpr int kStreamDelay = 31;       // D, input frames
constexpr int kStreamMaxL = 441;
constexpr int kStreamMinRate = 8000, kStreamMaxRate = 48000;
constexpr int kStreamTile = 256;       // outputs a workgroup of the kernel forms
// floats of input a tile of kStreamTile outputs reads at most: M / L <= 48000 / 44100, so its outputs span at most
// floor(255 * 160 / 147 + 146 / 147) + 1 = 279 positions, and the first reaches 63 frames back
constexpr int kStreamSpanMax = 344;

// L and M of a rate; false: the rate is not accepted
JF_STREAM_HD bool stream_ratio(int rate, int *L, int *M) {
    if (rate < kStreamMinRate || rate > kStreamMaxRate) return false;
    int a = rate, b = kStreamOutRate;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    const int l = kStreamOutRate / a, m = rate / a;
    if (l > kStreamMaxL) return false;
    *L = l;
    *M = m;
    return true;
}

// i(t) for t >= -1 (t M < 2^63 for every t below 2^53)
JF_STREAM_HD long long stream_index(long long t, int L, int M) { return t < 0 ? -1 : (t * (long long)M) / L; }
JF_STREAM_HD int stream_phase(long long t, int L, int M) { return (int)((t * (long long)M) % L); }
JF_STREAM_HD long long stream_need(long long t0, long long n, int L, int M) {
    return n <= 0 ? 0 : stream_index(t0 + n - 1, L, M) - stream_index(t0 - 1, L, M);
}
// the most frames a call of n outputs can need, whatever its t0
JF_STREAM_HD long long stream_need_max(long long n, int L, int M) { return (n * (long long)M + L - 1) / L; }

// One output from its 64 taps: h = the phase's row, x = a pointer to x[i] with x[-1] .. x[-63] valid behind it.
JF_STREAM_HD float stream_dot(const float *h, const float *x) {
    JF_STREAM_NO_CONTRACT
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int k = 0; k < kStreamTaps; k += 4) {
        const float m0 = h[k] * x[-k];
        const float m1 = h[k + 1] * x[-(k + 1)];
        const float m2 = h[k + 2] * x[-(k + 2)];
        const float m3 = h[k + 3] * x[-(k + 3)];
        a0 = a0 + m0;
        a1 = a1 + m1;
        a2 = a2 + m2;
        a3 = a3 + m3;
    }
    return (a0 + a1) + (a2 + a3);
}

}  // namespace jf
