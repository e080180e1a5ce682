// jf_room.h -- what the room stage's kernels (jf_room.hip) and their schedule (jf_engine_room.cpp) share: one launch
// parameter block.  The room is an auxiliary send (include/jefferson.h: jf_room_set_ir): per output bus the
// sum of its sources' scaled inputs, convolved with one stereo response by uniformly partitioned overlap-save (partitions of
// one block of B samples), added to the bus's mix behind the spatialiser.  ONE delay line per bus, TWO responses.
#ifndef JF_ROOM_H
#define JF_ROOM_H

#include "jf_device.h"

namespace jf {

struct RoomParams {
    const SrcSignal *sigs;   // [S] the sources' ordinary records (a follower's is a copy of its root's, a live source's its ring)
    const SrcState *st_in;   // [S] play positions of the call's state parity
    const int *seg;          // [n_buses + 1] offsets into list / lv
    const int *list;         // the sending sources, bus by bus, ascending within a bus
    const float2 *lv;        // per entry of list: (l_prev, l_new)
    float *send;             // [n_buses][K][B] the call's send blocks
    const float *prev_in;    // [n_buses][B] the last send block of the call before
    float *prev_out;         // [n_buses][B] ... of this call (the other buffer of the pair)
    const float2 *tw;        // exp(+2 pi i j / 1024), j < 1024
    float2 *fdl;             // [n_buses][Rg][B] the delay lines: packed spectra of [previous block | block]
    const float2 *hspec;     // [1 or 2][hstride] the responses' packed spectra, pre-scaled by gain / B: [P][B] each
    float *wet;              // [n_buses][K][2B] the call's wet blocks, interleaved stereo
    int n_buses, K, B;
    int P;                   // partitions of B taps
    int Rg;                  // slots of a delay line (P + max_batch_blocks)
    int head;                // slot block 0 of the call goes to
    int hstride;             // float2 between the two responses (even: 16-byte loads)
    int mono;                // 1: one response, heard on both ears
};

}  // namespace jf

#endif  // JF_ROOM_H
