// freeverb_params.hpp — what the host derives for a Freeverb before any sample is ticked: the 24 line lengths and the seven doubles the
// kernels read.  One statement of it for both users: the flattener (OP_FREEVERB, a reverb inside the per-voice graph) and the bus
// reverbs (srack_buses_set_reverb, a reverb behind a mix bus).  The freeverb crate's Freeverb::new / set_*, restated (see
// oracle/srack_oracle.c for what the restatement rests on).
#pragma once
#include <cstdint>

#include "../../include/srack_hip.h"
#include "program.hpp"

namespace srack {

// The shortest line (the last left allpass, tuning 225) must hold the four samples the tile function reads at a time: 784 Hz.
constexpr uint32_t kFvMinLine = 4;

// Line j = 2 * unit + channel (units 0..7 combs, 8..11 allpasses); adjust_length: `(length as f64 * sr as f64 / 44100.0) as usize`, the
// right channel's tuning the left's plus 23 (stereo spread).  first[j]: where line j starts when the lines lie back to back.
// Returns false when a line comes out shorter than kFvMinLine (a zero-length line panics in the crate).
inline bool fv_line_lengths(uint32_t sample_rate, uint32_t len[kFvLines], uint32_t first[kFvLines], uint32_t* total_out)
{
    static const uint32_t comb_tuning[8] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, allpass_tuning[4] = {556, 441, 341, 225};
    uint32_t total = 0;
    for (int j = 0; j < kFvLines; j++) {
        const uint32_t tuning = (j < 16 ? comb_tuning[j / 2] : allpass_tuning[(j - 16) / 2]) + ((j & 1) ? 23u : 0u);
        len[j] = (uint32_t)((double)tuning * (double)sample_rate / 44100.0);
        if (len[j] < kFvMinLine) return false;
        first[j] = total;
        total += len[j];
    }
    if (total_out) *total_out = total;
    return true;
}

// Freeverb::new's defaults, then set_freeverb(all = true) in its order (freeverb.rs:88-114): every setter runs once.  Each derived
// value depends on the current six fields alone, so the slider path (set_freeverb(false): only the changed setters run) gives the same.
// fields: the module's six in field order (SRACK_FREEVERB_*); par: comb feedback, comb dampening, 1 - dampening, wet_gains.0,
// wet_gains.1, dry, input_gain.
inline void fv_derive(const double fields[SRACK_FREEVERB__NFIELDS], double par[7])
{
    const double dampening = fields[SRACK_FREEVERB_DAMPENING] * 0.4, room = fields[SRACK_FREEVERB_ROOM_SIZE] * 0.28 + 0.7;
    const bool frozen = fields[SRACK_FREEVERB_FREEZE] != 0.0;
    const double wet = fields[SRACK_FREEVERB_WET] * 3.0, width = fields[SRACK_FREEVERB_WIDTH];
    const double comb_damp = frozen ? 0.0 : dampening;
    par[0] = frozen ? 1.0 : room;
    par[1] = comb_damp;
    par[2] = 1.0 - comb_damp;
    par[3] = wet * (width / 2.0 + 0.5);
    par[4] = wet * ((1.0 - width) / 2.0);
    par[5] = fields[SRACK_FREEVERB_DRY];
    par[6] = 1.0;  // input_gain: set by new(); the public set_freeze leaves it alone
}

}  // namespace srack
