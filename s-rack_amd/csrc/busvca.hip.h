// busvca.hip.h — the bus VCAs (srack_buses_vca): an ADSRModule and a VCAModule per channel on every mix bus, behind the mixer.
//
// Bus b has one control row ctl[b][t].  In mode GATE it is the Gate input of one ADSRModule (adsr.rs:134-217) whose output is the CV of
// the bus's VCAs; in mode CV it is that CV itself; a bus that is OFF passes.  Channel c (0 or 1) of the bus is one VCAModule
// (vca.rs:117-148): audio rows[b][c][t] in, out[b][c][t] out.  The unit is built with -ffp-contract=off: every operation is the
// reference's f32 operation, one rounding each (modules.hip.h: adsr_consts, adsr_seg_step — the segmented form of adsr_step, the same
// operations between two changes of mode, adsr_step itself on the sample that may change it —, vca_step).
//
// The work has two shapes, and a workgroup of eight waves per 64 buses gives each its own.
//   the envelope  is serial in time and exists once per bus.  Lane l of the workgroup's FIRST wave is bus b0 + l; its state stays in that
//                 wave's registers for the whole call.  The control rows are time-minor in memory, so a tile of 64 buses x 64 samples is
//                 loaded with lanes on time (whole 256-byte pieces, eight buses per wave), turned through LDS — word j * 65 + k: the odd
//                 stride puts a column of 32 buses on 32 banks — walked by the first wave, eight samples read ahead of the eight being
//                 computed, and the envelope is written back into the tile's own words.  A bus that is not GATE keeps its words: the CV,
//                 or +0.0.  The eight samples are asked about at once: if no lane leaves its segment on any of them (one ballot), they
//                 are the segment's add and multiply-add and nothing else; otherwise they go through adsr_seg_step one by one.
//   the VCA       is elementwise: lanes stay on time.  Each wave takes eight of the tile's buses: per bus and used channel one coalesced
//                 load, the envelope (or CV) word out of the tile, vca_step, one coalesced store; env comes straight out of the tile.
//                 The audio never passes through LDS, the envelope never through memory unless env asks for it.
// Memory runs a tile ahead: tile i + 1's loads — control words first, then audio — are issued before tile i's serial stage and wait in
// registers behind it and behind tile i's stores, so that a workgroup alone on its CU (a small console) pays a tile's round trip to memory
// once per call, not once per tile.
// A workgroup none of whose buses is GATE skips the turn, the serial stage and every barrier (wave-uniformly): a plain streaming pass,
// the control word going from its load straight into vca_step.  An OFF bus's words are copied out of place and left alone in place.
// In place (out == rows) is safe: a word is read and written by the same lane, read first.  Tails — a last tile under 64 samples, a last
// group under 64 buses — are masked, never padded.  Nothing needs more than 4-byte alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bustile.hip.h"
#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusVcaTile = kRowTile;          // samples per tile, and buses per workgroup: the tile's geometry is bustile.hip.h's,
constexpr int kBusVcaStride = kRowTileStride;  // LDS words per bus of the tile; the pipeline around it is this kernel's own
#ifndef SRACK_BUSVCA_WAVES           // (variants of the three choices below were built to measure them: notes/r20.md)
#define SRACK_BUSVCA_WAVES 8
#endif
#ifndef SRACK_BUSVCA_NEXT_AHEAD
#define SRACK_BUSVCA_NEXT_AHEAD 1
#endif
#ifndef SRACK_BUSVCA_CHUNK
#define SRACK_BUSVCA_CHUNK 8
#endif
constexpr int kBusVcaWaves = SRACK_BUSVCA_WAVES;  // waves per workgroup; the first one also walks the envelopes
constexpr bool kBusVcaNextAhead = SRACK_BUSVCA_NEXT_AHEAD != 0;  // the NEXT tile's loads are issued before this tile's serial stage (else behind it)
constexpr int kBusVcaShare = kBusVcaTile / kBusVcaWaves;  // buses of the tile a wave streams
constexpr int kBusVcaAhead = SRACK_BUSVCA_CHUNK;  // samples the serial stage reads from LDS at a time, and asks about at once
static_assert(kBusVcaTile % kBusVcaWaves == 0 && kBusVcaTile % kBusVcaAhead == 0, "whole shares, whole chunks");
static_assert(kBusVcaFields == SRACK_BUS_VCA_NSTATE && SRACK_ADSR_GATE_LAST - SRACK_ADSR_PHASE + 1 == SRACK_BUS_VCA_NSTATE, "the state is SRACK_ADSR_PHASE .. SRACK_ADSR_GATE_LAST, as the C ABI hands it out");

// grid (ceil(n_buses / 64)), block 512 (two workgroups per CU: 128 VGPRs).  kUsed: a.used, 1 or 2 — the channels of a bus that are processed.
template <int kUsed>
__global__ __launch_bounds__(kBusVcaWaves * 64, kBusVcaWaves / 2) void bus_vca(const BusVcaArgs a)
{
    using namespace dev;
    __shared__ uint32_t s_e[kBusVcaTile * kBusVcaStride];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t b0 = blockIdx.x * (uint32_t)kBusVcaTile;
    const uint32_t live = min((uint32_t)kBusVcaTile, a.n_buses - b0);  // buses of this workgroup
    // every wave holds the group's 64 (mode, negative) pairs, lane l bus b0 + l; a lane past the last bus reads as OFF
    const bool exists = lane < live;
    const BusVcaBus me = a.tab[b0 + (exists ? lane : 0u)];
    const uint32_t my_flags = exists ? (me.mode | (me.negative ? 4u : 0u)) : (uint32_t)SRACK_BUS_VCA_OFF;
    const bool gated = (my_flags & 3u) == (uint32_t)SRACK_BUS_VCA_GATE;
    const bool any_gate = __builtin_amdgcn_ballot_w64(gated) != 0;     // the same in every wave
    const bool serial = any_gate && wave == 0;
    const bool in_place = a.out == a.rows;
    const uint32_t* rows = reinterpret_cast<const uint32_t*>(a.rows);
    const uint32_t* ctl = reinterpret_cast<const uint32_t*>(a.ctl);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out);
    uint32_t* env = reinterpret_cast<uint32_t*>(a.env);

    // the first wave's envelopes: loaded once, stored once (f32 [kBusVcaFields][n_buses], as the C ABI hands the values out)
    AdsrRegs s;
    s.phase = 0.0f, s.r_val = 0.0f, s.from_a_val = 0.0f, s.mode = SRACK_ADSR_MODE_NONE, s.gate_last = true;
    AdsrConst k = adsr_consts(me.a_sec, me.d_sec, me.s_val, me.r_sec, a.rate);
    AdsrSeg g;
    if (serial) {
        if (gated) {
            const float* st = a.state + b0 + lane;
            s.phase = st[0 * (size_t)a.n_buses];
            s.mode = (int)st[1 * (size_t)a.n_buses];
            s.r_val = st[2 * (size_t)a.n_buses];
            s.from_a_val = st[3 * (size_t)a.n_buses];
            s.gate_last = st[5 * (size_t)a.n_buses] != 0.0f;
        }
        adsr_seg_enter(s, k, g);
    }

    // A wave's share of a tile, lanes on time: its control words first — the serial stage waits for those alone (loads return in the order
    // they were issued) —, then its audio, which the VCAs want only behind that stage.  A tile past the end loads nothing.
    auto load_tile = [&](uint32_t t0, uint32_t (&c_)[kBusVcaShare], uint32_t (&x_)[kBusVcaShare][kUsed]) {
        const bool in_time = t0 < a.n && lane < a.n - t0;
#pragma unroll
        for (int q = 0; q < kBusVcaShare; q++) {
            const uint32_t j = wave * kBusVcaShare + q;
            const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)my_flags, (int)j);
            c_[q] = 0u;  // +0.0: an OFF bus, a bus past the last one, no control row
            if (ctl && (f & 3u) != (uint32_t)SRACK_BUS_VCA_OFF && in_time) c_[q] = (ctl + ((size_t)(b0 + j) * a.n + t0))[lane];
        }
#pragma unroll
        for (int q = 0; q < kBusVcaShare; q++) {
            const uint32_t j = wave * kBusVcaShare + q;
            const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)my_flags, (int)j);
#pragma unroll
            for (int c = 0; c < kUsed; c++) {
                x_[q][c] = 0u;
                if (j < live && in_time && !((f & 3u) == (uint32_t)SRACK_BUS_VCA_OFF && in_place)) x_[q][c] = (rows + (((size_t)(b0 + j) * a.row_channels + c) * a.n + t0))[lane];
            }
        }
    };

    const uint32_t n_tiles = (a.n + kBusVcaTile - 1) / kBusVcaTile;
    uint32_t cw[kBusVcaShare], x[kBusVcaShare][kUsed];
    load_tile(0, cw, x);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kBusVcaTile;
        const uint32_t len = min((uint32_t)kBusVcaTile, a.n - t0);
        const bool in_time = lane < len;
        uint32_t cn[kBusVcaShare], xn[kBusVcaShare][kUsed];  // tile i + 1, in flight behind tile i's serial stage and stores
        if (any_gate) {
#pragma unroll
            for (int q = 0; q < kBusVcaShare; q++) s_e[(wave * kBusVcaShare + q) * kBusVcaStride + lane] = cw[q];
            __syncthreads();
            if (kBusVcaNextAhead) load_tile(t0 + kBusVcaTile, cn, xn);
            if (serial) {
                // lane l walks bus l's samples: kBusVcaAhead of them are read out of the tile ahead of the ones being computed
                const uint32_t at = lane * kBusVcaStride;
                float gt[kBusVcaAhead];
#pragma unroll
                for (int q = 0; q < kBusVcaAhead; q++) gt[q] = __uint_as_float(s_e[at + q]);
                for (uint32_t k0 = 0; k0 < len; k0 += kBusVcaAhead) {
                    float gn[kBusVcaAhead];
                    const uint32_t next = min(k0 + kBusVcaAhead, (uint32_t)(kBusVcaTile - kBusVcaAhead));  // (the last chunk reads itself again: no branch)
#pragma unroll
                    for (int q = 0; q < kBusVcaAhead; q++) gn[q] = __uint_as_float(s_e[at + next + q]);
                    // A quiet chunk: no lane leaves its segment on any of its samples — by the gates' levels and edges, which every lane
                    // sums up for its own row, and by the phase, which stays below 1 (adsr_seg_quiet's bound: each rounded addition adds at
                    // most inc + 2^-24) — asked once, with one ballot.  Its samples are the segment's own operations and nothing else
                    // (adsr_seg_quiet_step: what adsr_seg_step does when nobody leaves).  Any other chunk goes sample by sample.
                    bool quiet = false;
                    if (k0 + kBusVcaAhead <= len) {  // (wave-uniform)
                        bool prev = lane_bit(g.last), any_high = false, any_low = false, any_edge = false;
#pragma unroll
                        for (int q = 0; q < kBusVcaAhead; q++) {
                            const bool h = gated && gt[q] > 0.0f;  // (a NaN gate is not high: it counts as low here, and Sustain then asks sample by sample)
                            any_high = any_high || h, any_low = any_low || !h, any_edge = any_edge || (h && !prev);
                            prev = h;
                        }
                        const bool leave = (lane_bit(g.on_high) && any_high) || (lane_bit(g.on_low) && any_low) || (lane_bit(g.on_edge) && any_edge) ||
                                           !(s.phase + (float)kBusVcaAhead * g.inc <= 0.9999f);
                        quiet = __builtin_amdgcn_ballot_w64(leave) == 0;
                        if (quiet) {
#pragma unroll
                            for (int q = 0; q < kBusVcaAhead; q++) {
                                const float e = adsr_seg_quiet_step(s, g);
                                if (gated) s_e[at + k0 + q] = __float_as_uint(e);  // (a bus that is not GATE keeps its words)
                            }
                            g.last = __builtin_amdgcn_ballot_w64(prev);
                        }
                    }
                    if (!quiet) {
#pragma unroll
                        for (int q = 0; q < kBusVcaAhead; q++) {
                            if (k0 + q < len) {  // (wave-uniform)
                                const float e = adsr_seg_step(s, k, g, gated ? gt[q] : 0.0f);  // a lane without an envelope idles in mode None
                                if (gated) s_e[at + k0 + q] = __float_as_uint(e);
                            }
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kBusVcaAhead; q++) gt[q] = gn[q];
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kBusVcaShare; q++) cw[q] = s_e[(wave * kBusVcaShare + q) * kBusVcaStride + lane];
            __syncthreads();  // (the next tile's words go into the same place)
            if (!kBusVcaNextAhead) load_tile(t0 + kBusVcaTile, cn, xn);
        } else {
            load_tile(t0 + kBusVcaTile, cn, xn);
        }
        if (in_time) {
#pragma unroll
            for (int q = 0; q < kBusVcaShare; q++) {
                const uint32_t j = wave * kBusVcaShare + q;
                if (j >= live) break;  // (wave-uniform)
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)my_flags, (int)j);
                const uint32_t b = b0 + j, m = f & 3u;
                if (env) (env + ((size_t)b * a.n + t0))[lane] = cw[q];
                if (m == (uint32_t)SRACK_BUS_VCA_OFF) {
                    if (!in_place) {
#pragma unroll
                        for (int c = 0; c < kUsed; c++) (out + (((size_t)b * a.row_channels + c) * a.n + t0))[lane] = x[q][c];
                    }
                    continue;
                }
                // a CV bus without a control row: the VCA's CV port is unconnected, output.fill(0.0)
                const uint32_t fl = (m == (uint32_t)SRACK_BUS_VCA_CV && !ctl) ? VCA_HAS_AUDIO : (VCA_HAS_AUDIO | VCA_HAS_CV);
#pragma unroll
                for (int c = 0; c < kUsed; c++)
                    (out + (((size_t)b * a.row_channels + c) * a.n + t0))[lane] = __float_as_uint(vca_step(fl, (f & 4u) != 0, __uint_as_float(x[q][c]), __uint_as_float(cw[q])));
            }
        }
#pragma unroll
        for (int q = 0; q < kBusVcaShare; q++) {
            cw[q] = cn[q];
#pragma unroll
            for (int c = 0; c < kUsed; c++) x[q][c] = xn[q][c];
        }
    }

    if (serial) {
        adsr_seg_flush(s, g);
        if (gated) {
            float* st = a.state + b0 + lane;
            st[0 * (size_t)a.n_buses] = s.phase;
            st[1 * (size_t)a.n_buses] = (float)s.mode;
            st[2 * (size_t)a.n_buses] = s.r_val;
            st[3 * (size_t)a.n_buses] = s.from_a_val;
            st[5 * (size_t)a.n_buses] = s.gate_last ? 1.0f : 0.0f;
        }
    }
}

}  // namespace srack
