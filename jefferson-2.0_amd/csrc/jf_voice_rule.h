// jf_voice_rule.h -- the VOICE LIMIT rule (include/jefferson.h: "voice limits"): which of a bus's sources are
// heard in a block when the bus renders at most N of them.  Compiled for BOTH sides in the manner of jf_gate_rule.h and
// jf_master_rule.h: the kernels (jf_voice.hip) and the host (jf_debug_voice_select, which the CPU suite checks case by case)
// include this one file and get the same bits.  Self-contained: a plain C++ compiler can build it, and it calls no libm function.
//
// Per bus b: max_voices N_b (0: no limit, the default; 0 .. kVoiceMax) and release rho_b (float32, 0 <= rho < 1, default 0).
// Per source: a priority 0 .. 255 (default 0; 255 = kVoiceAlways: always heard, takes no place) and a state {env_prev, initially
// 0; heard_prev, initially 1 -- before a limit existed everybody was heard}.
//
// THE ENVELOPE of block k, from the level p[k] the gate stage measures (jf_gate_rule.h: the peak of what the block appends to
// the source's input; a follower reads its root's), with b the source's bus in this run:
//     d = fl32(env[k - 1] * rho_b);   env[k] = p >= d ? p : d;   env[k] < 2^-60: env[k] = 0
// One float32 product and one comparison; the stored value is never a denormal; rho = 0: the block's own peak.  The envelope of
// EVERY source advances in every run of an active engine, whatever its bus.
//
// CANDIDATES.  Source s is a candidate in block k if g_eff[k][s] != 0 (what gate_scan_kernel wrote: a closed gate, a mute or a
// zero gain is no candidate) and its priority is below 255.  THE RANKING of one bus's candidates: priority, higher first; then
// env[k], higher first, float32 compared as stored; then the source index, lower first.  rank = the number of candidates on the
// bus that come before the source.  keep[k][s] = 1 on a bus with N_b = 0; 1 for an ALWAYS source; candidate && rank < N_b on a
// limited bus (no candidate there: 0).
//
// WHAT THE GAIN STAGE SEES (jf_gain_rule.h, unchanged):  g_out[k][s] = keep[k][s] ? g_eff[k][s] : 0, and
// g_out[-1][s] = (N_b == 0 || ALWAYS || heard_prev[s]) ? g_eff[-1][s] : 0.  After the run heard_prev := keep of its last block and
// env_prev := env of that block.  With every keep at 1, g_out is g_eff bit for bit.  CONSEQUENCES:
//   - raising N, or a louder talker, ramps the new winner in from 0 over one block (kernels.cu:132-137): the gate's "the ramp on
//     opening is accepted" applies; a loser ramps out over one block; a block unheard at both ends is skipped;
//   - taking a limit away (N = 0) lets everybody in at once, as taking a gate away does;
//   - room sends are pre-fader and are not limited;
//   - a tie is only possible between sources that play one input, or by coincidence of peaks: the lower index wins it, the same
//     way every block.
// A setting made with fade == 0 has the first run that latches it take heard_prev as 0 for every source of that bus that is not
// ALWAYS (voice_heard_before's `snap`): losers are silent from the first sample and winners ramp in.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_VOICE_HD __host__ __device__ __forceinline__
#else
#define JF_VOICE_HD inline
#endif
#if defined(__clang__)
#define JF_VOICE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_VOICE_NO_CONTRACT
#endif

namespace jf {

constexpr int kVoiceMax = 65536;      // the largest max_voices a setter takes
constexpr int kVoiceAlways = 255;     // JF_VOICE_ALWAYS
constexpr float kVoiceEnvMin = 8.673617379884035e-19f;  // 2^-60: an envelope below it is stored as 0

// a bus's parameters as the device holds them, 16 bytes
struct VoiceBus {
    int max_voices;
    float release;
    int snap;  // the setting was made with fade == 0 and this call is the first to latch it
    int pad;
};

JF_VOICE_HD float voice_env_step(float env_prev, float p, float release) {
    JF_VOICE_NO_CONTRACT
    const float d = env_prev * release;
    const float env = p >= d ? p : d;
    return env < kVoiceEnvMin ? 0.0f : env;
}

JF_VOICE_HD bool voice_candidate(float g_eff, int priority) {
    JF_VOICE_NO_CONTRACT
    return g_eff != 0.0f && priority < kVoiceAlways;
}

JF_VOICE_HD unsigned voice_float_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    union {
        float f;
        unsigned u;
    } c;
    c.f = v;
    return c.u;
#endif
}

// The ranking key of a candidate: bit 63 (a candidate at all), priority in bits 32 .. 39, the envelope's bits below -- an
// envelope is never negative and never a NaN, so its bits order as its value does.  0: no candidate.  The source index is compared
// apart (voice_before), so the key holds for any number of sources.
JF_VOICE_HD unsigned long long voice_key(bool candidate, int priority, float env) {
    if (!candidate) return 0ull;
    return (1ull << 63) | ((unsigned long long)(unsigned)priority << 32) | (unsigned long long)voice_float_bits(env);
}

// does the source with key_a and index a come before the CANDIDATE or non-candidate with key_b and index b?  Only candidates
// come before anybody.
JF_VOICE_HD bool voice_before(unsigned long long key_a, int a, unsigned long long key_b, int b) {
    return (key_a >> 63) != 0 && (key_a > key_b || (key_a == key_b && a < b));
}

JF_VOICE_HD int voice_keep(int max_voices, int priority, bool candidate, int rank) {
    if (max_voices == 0 || priority >= kVoiceAlways) return 1;
    return candidate && rank < max_voices ? 1 : 0;
}

// was the source heard in the block before the run, as g_out[-1] asks?
JF_VOICE_HD bool voice_heard_before(int max_voices, int priority, int heard_prev, int snap) {
    if (max_voices == 0 || priority >= kVoiceAlways) return true;
    return snap ? false : heard_prev != 0;
}

// what the setters accept
JF_VOICE_HD bool voice_params_ok(int max_voices, float release) {
    JF_VOICE_NO_CONTRACT
    if (max_voices < 0 || max_voices > kVoiceMax) return false;
    return release >= 0.0f && release < 1.0f;  // (a NaN fails both)
}
JF_VOICE_HD bool voice_priority_ok(int priority) { return priority >= 0 && priority <= kVoiceAlways; }

}  // namespace jf
