// jf_desc_edit.hip -- the two kernels that edit a batch run's descriptors in place: desc_set_kernel (HRTF sets; include/jefferson.h:
// jf_engine_add_hrtf_set, jf_source_set_hrtf) and, behind it, desc_gain_kernel (per-source gain:
// jf_source_set_gain, jf_batch_set_gains).  Both are desc_edit_wave (jf_desc_edit.h: the scheme) around the rule
// for one record -- jf_set_rule.h, jf_gain_rule.h, compiled here and in the engine's host side: the same bits.  Each is launched
// only while its control is active; NEITHER is idempotent -- once per run, on the buffer the run takes.
//
// Gain: g_prev[S], g_new[S], g_traj[K][S] or null.  Item (k, s): g1 = g[k] = g_traj ? g_traj[k][s] : g_new[s]; g0 = g[k - 1] =
// g_prev[s] for k == 0, else g_traj ? g_traj[k - 1][s] : g_new[s].  Neutral: 1.  May write w_new, rows_old, w_old, n_new, n_old,
// flags -- never rows_new.  Nothing is read outside g_prev / g_new[0 .. S), g_traj[0 .. K S).
//
// Sets: set_prev[S] (null: every source's set_new), set_new[S], n_rows.  Item (k, s): off1 = set_new[s] n_rows; off0 =
// set_prev[s] n_rows for k == 0, else off1 -- only the first block of a call's first run sees the set before.  Neutral: set 0.
// May write rows_new, rows_old, w_old, n_old, flags -- never w_new or n_new.  Nothing is read outside set_prev / set_new[0 .. S).
#include "jf_desc_edit.h"
#include "jf_gain_rule.h"
#include "jf_set_rule.h"

namespace jf {

namespace {

struct GainEdit {
    using Value = float;
    static constexpr float kNeutral = 1.0f;
    static constexpr unsigned kWordMask = 0x0000fff0u | (7u << kNNew);  // words 4 .. 15 and 19 .. 21
    const float *g_prev, *g_new, *g_traj;
    int S;
    __device__ __forceinline__ EditPair<float> load(int item, int k, int s) const {
        const float g1 = g_traj != nullptr ? g_traj[item] : g_new[s];
        const float g0 = k == 0 ? g_prev[s] : (g_traj != nullptr ? g_traj[item - S] : g_new[s]);
        return {g0, g1};
    }
    __device__ __forceinline__ bool apply(DescRecord &d, float g0, float g1, int canon) const { return gain_rule(d, g0, g1, canon); }
    static __device__ __forceinline__ void put(unsigned *r, const DescRecord &d) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            r[kWNew + t] = __float_as_uint(d.w_new[t]);
            r[kRowsOld + t] = (unsigned)d.rows_old[t];
            r[kWOld + t] = __float_as_uint(d.w_old[t]);
        }
        r[kNNew] = (unsigned)d.n_new;
        r[kNOld] = (unsigned)d.n_old;
        r[kFlags] = (unsigned)d.flags;
    }
};

struct SetEdit {
    using Value = int;
    static constexpr int kNeutral = 0;
    static constexpr unsigned kWordMask = 0x0000ff0fu | (3u << kNOld);  // words 0 .. 3, 8 .. 15, 20 and 21
    const int *set_prev, *set_new;
    int n_rows;
    __device__ __forceinline__ EditPair<int> load(int, int k, int s) const {
        const int j1 = set_new[s];
        const int j0 = k == 0 && set_prev != nullptr ? set_prev[s] : j1;
        return {j0, j1};
    }
    __device__ __forceinline__ bool apply(DescRecord &d, int j0, int j1, int canon) const {
        return set_rule(d, j0 * n_rows, j1 * n_rows, canon);  // (set < JF_MAX_HRTF_SETS, n_rows <= 16384: far from overflow)
    }
    static __device__ __forceinline__ void put(unsigned *r, const DescRecord &d) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            r[kRowsNew + t] = (unsigned)d.rows_new[t];
            r[kRowsOld + t] = (unsigned)d.rows_old[t];
            r[kWOld + t] = __float_as_uint(d.w_old[t]);
        }
        r[kNOld] = (unsigned)d.n_old;
        r[kFlags] = (unsigned)d.flags;
    }
};

__global__ __launch_bounds__(kEditThreads) void desc_gain_kernel(ItemDesc *__restrict__ desc, const float *__restrict__ g_prev,
                                                                 const float *__restrict__ g_new, const float *__restrict__ g_traj,
                                                                 int S, int total /* K S */, int canon) {
    desc_edit_wave(desc, total, S, canon, GainEdit{g_prev, g_new, g_traj, S});
}

__global__ __launch_bounds__(kEditThreads) void desc_set_kernel(ItemDesc *__restrict__ desc, const int *__restrict__ set_prev,
                                                                const int *__restrict__ set_new, int S, int total /* K S */,
                                                                int n_rows, int canon) {
    desc_edit_wave(desc, total, S, canon, SetEdit{set_prev, set_new, n_rows});
}

// what both launches check, and their grid: a wave per 64 records, the item index an int with room to spare
bool edit_grid(const ItemDesc *d_desc, int S, int K, dim3 *grid, int *total) {
    if (S <= 0 || K <= 0 || !d_desc) return false;
    const long long n = (long long)S * K;
    if (n > 0x7fffffffLL / 32 || ((size_t)d_desc & 7)) return false;
    *grid = dim3((unsigned)((n + kEditThreads - 1) / kEditThreads));
    *total = (int)n;
    return true;
}

}  // namespace

// d_desc [K][S] (the buffer the run takes), d_g_prev / d_g_new [S], d_g_traj [K][S] or null
hipError_t launch_desc_gain(ItemDesc *d_desc, const float *d_g_prev, const float *d_g_new, const float *d_g_traj, int S, int K,
                            int canon, hipStream_t st) {
    dim3 grid;
    int total;
    if (!d_g_prev || !d_g_new || !edit_grid(d_desc, S, K, &grid, &total)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(desc_gain_kernel, grid, dim3(kEditThreads), 0, st, d_desc, d_g_prev, d_g_new, d_g_traj, S, total, canon);
    return hipGetLastError();
}

// d_desc [K][S] (the buffer the run takes), d_set_prev [S] or null (no source changes its set in this run), d_set_new [S]
hipError_t launch_desc_set(ItemDesc *d_desc, const int *d_set_prev, const int *d_set_new, int S, int K, int n_rows, int canon,
                           hipStream_t st) {
    dim3 grid;
    int total;
    if (n_rows <= 0 || !d_set_new || !edit_grid(d_desc, S, K, &grid, &total)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(desc_set_kernel, grid, dim3(kEditThreads), 0, st, d_desc, d_set_prev, d_set_new, S, total, n_rows, canon);
    return hipGetLastError();
}

}  // namespace jf
