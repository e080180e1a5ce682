// jf_gate_rule.h -- the VOICE GATE rule (include/jefferson.h: "voice gates"): whether a source is heard in a
// block, from the level of what that block appends to its input.  Compiled for BOTH sides in the manner of jf_gain_rule.h and
// jf_master_rule.h: the kernels (jf_gate.hip) and the host (jf_debug_gate_scan, which the CPU suite checks case by case)
// include this one file and get the same bits.  Self-contained: a plain C++ compiler can build it.
//
// Per source: open (a float32 linear peak; 0: no gate, always heard), close (0 <= close <= open), hold (whole blocks,
// 0 .. kGateHoldMax) and a state {is_open, hold_left}, closed with hold_left = 0 at first.  The level of block k is
// p = max |x| over the B samples the block appends to the source's INPUT (pre-fader; exact in float32 and independent of the
// order of the reduction).  THE RULE for one block, in this order:
//   1. p >= open                      is_open = 1, hold_left = hold
//   2. else is_open and p >= close    hold_left = hold
//   3. else is_open and hold_left > 0 hold_left -= 1
//   4. else                           is_open = 0
// gate[k] = is_open after the step.  A source without a gate has gate[k] = 1 and its state is not touched.  Every comparison is
// a float32 comparison of values as stored: no arithmetic on the levels at all, so nothing a contraction setting could change --
// the functions carry the pragma like the other rules.
//
// What the gate does to the audio is the gain rule's (jf_gain_rule.h), fed g_eff[k] = gate[k] ? g[k] : 0 in place of g[k], with
// g_eff[-1] = (open before the run ? g[-1] : 0): an OPENING gate is the reference's one-block crossfade from 0
// (kernels.cu:132-137), a closing one the same ramp to 0, a block closed at both ends is skipped, an open gate multiplies by
// nothing.  THE RAMP ON OPENING IS ACCEPTED: the block whose level opens the gate fades in over its B samples, so the first
// milliseconds of an onset are attenuated.  There is no look-ahead or pre-roll (a run must give the same bits however it is
// cut into calls) and no attack or release time other than one block.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_GATE_HD __host__ __device__ __forceinline__
#else
#define JF_GATE_HD inline
#endif
#if defined(__clang__)
#define JF_GATE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_GATE_NO_CONTRACT
#endif

namespace jf {

constexpr int kGateHoldMax = 1048576;  // blocks

struct GateState {
    int is_open;
    int hold_left;
};

// a source's parameters as the device holds them, 16 bytes
struct GatePar {
    float open;
    float close;
    int hold;
    int pad;
};

JF_GATE_HD float gate_abs(float v) { return v < 0.0f ? -v : v; }
// (a NaN sample never raises a level: the comparison is false)
JF_GATE_HD float gate_max(float a, float b) { return b > a ? b : a; }

// one block of a source WITH a gate (open > 0); the gate of the block
JF_GATE_HD int gate_step(GateState &st, float p, float open, float close, int hold) {
    JF_GATE_NO_CONTRACT
    if (p >= open) {
        st.is_open = 1;
        st.hold_left = hold;
    } else if (st.is_open && p >= close) {
        st.hold_left = hold;
    } else if (st.is_open && st.hold_left > 0) {
        st.hold_left -= 1;
    } else {
        st.is_open = 0;
    }
    return st.is_open;
}

// The largest threshold a setter takes: 2^24, 144 dB over the full scale of 1.  No input that the engine can render reaches it,
// so a larger one can only mean "never" -- and a call with garbage arguments must not silence every source for good (the
// thresholds outlive jf_source_set_signal and jf_source_reset; jf_bus_set_master refuses 0 for the same reason).
constexpr float kGateOpenMax = 16777216.0f;

// what the setters accept: 0 <= close <= open <= kGateOpenMax (hence finite), 0 <= hold <= kGateHoldMax
JF_GATE_HD bool gate_params_ok(float open, float close, int hold) {
    JF_GATE_NO_CONTRACT
    if (!(open >= 0.0f) || !(close >= 0.0f)) return false;  // negative or NaN
    if (!(open <= kGateOpenMax)) return false;               // infinite, or beyond anything a signal reaches
    return close <= open && hold >= 0 && hold <= kGateHoldMax;
}

}  // namespace jf
