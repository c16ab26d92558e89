// jit_gen.cpp — the general path's fast half: a voice kernel SPECIALISED for one flattened program.  This unit is the generator: a pure
// function from the program to a text (host code, no HIP); jit_cache.cpp compiles and caches the text, jit.cpp loads and launches it.
//
// The hand-matched fused kernels (fused.hip.h, seq.hip.h, fm_pair.hip.h, fm_block.hip.h) cover five patch shapes; the tile interpreter (interp.hip.h) covers everything
// but pays for its generality — every wire makes a round trip through LDS, every module is a call with its state loaded and
// stored per tile (P1 through it: 0.21 of the HBM roofline where the fused kernel reaches 0.57).  Here the flattened op list is
// turned into ONE straight-line HIP kernel over the very same per-module device functions (modules.hip.h): wires are
// registers, module state lives in registers for the whole launch, control tracks arrive through scalar loads, frames leave
// through buffer stores, the mix-down goes through the same LDS transpose tile as in the fused kernels (wave.hip.h).  The
// source is compiled for the device's architecture with hiprtc the first time a program STRUCTURE is seen (op kinds, flags,
// wiring, which parameters are per-voice rows; parameter values are read from the op list at run time) and cached.
//
// Reference semantics held: one calc() per planned module per sample in plan order (src/synth.rs:97-101); a broken feedback
// edge is a buffer_size-sample delay.  What the generator does not cover falls back to the interpreter
// (jit_supported): FreeverbModule (its 24 delay lines per voice live in HBM and have their own tile function).
#include "jit_gen.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

namespace srack {

namespace {

// ---- the experiment knobs (tools/): environment variables that change the generated text, for A/B runs -------------------------------
// Read once per jit_source call — so a host may change one between renders, as tests/test_gpu_planes.py does — and handed to every Gen.
// This table is the one place they are listed.  (SRACK_JIT_OPTS and SRACK_JIT_BUDGET are the cache's and jit_get's: not text.)
struct GenKnobs {
    bool quiet = true;            // SRACK_JIT_QUIET=0            the per-sample forms only: no quiet groups
    int nq_unroll = 8;            // SRACK_JIT_NQ_UNROLL=1..8     how far the per-sample copy of a quiet-group kernel is unrolled
    bool fm = true;               // SRACK_JIT_FM=0               every oscillator keeps the literal forms: no versioning on bounded pitch CVs
    bool across_lanes = true;     // SRACK_CTL_ACROSS_LANES=0     control units sample by sample, not a tile across the lanes
    bool smp_lds = true;          // SRACK_JIT_SMP_LDS=0          a sample player's wave is gathered through the global pointer, never staged in LDS
    bool smp_window = true;       // SRACK_JIT_SMP_WINDOW=0       the plain gather from a bank in global memory (tools/bank_bench.py)
    int unroll_cap = 0;           // SRACK_JIT_UNROLL=n >= 1      a cap on the unrolling of voice programs (0: none)
    int quiet_group = 0;          // SRACK_JIT_QUIET_GROUP=4|16   samples per quiet group, where not the device headers' 8 (0)
    bool waves_set = false;       // SRACK_JIT_WAVES=n            the register budget in waves per SIMD, overriding jit_get's
    int waves = 0;
    bool tile_per_plane = false;  // SRACK_TILE_PER_PLANE (set)   every output plane its own LDS mix tile, none shared row-wise
};

GenKnobs read_knobs()
{
    auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };  // a switch: "0" turns the path off
    auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
    GenKnobs k;
    k.quiet = on("SRACK_JIT_QUIET"), k.fm = on("SRACK_JIT_FM"), k.across_lanes = on("SRACK_CTL_ACROSS_LANES");
    k.smp_lds = on("SRACK_JIT_SMP_LDS"), k.smp_window = on("SRACK_JIT_SMP_WINDOW");
    const int nq = num("SRACK_JIT_NQ_UNROLL"), cap = num("SRACK_JIT_UNROLL"), group = num("SRACK_JIT_QUIET_GROUP");
    k.nq_unroll = nq >= 1 && nq <= 8 ? nq : 8;
    k.unroll_cap = cap >= 1 ? cap : 0;
    k.quiet_group = group == 4 || group == 16 ? group : 0;
    k.waves_set = getenv("SRACK_JIT_WAVES") != nullptr;
    k.waves = num("SRACK_JIT_WAVES");
    k.tile_per_plane = getenv("SRACK_TILE_PER_PLANE") != nullptr;
    return k;
}

// ---- code generation ---------------------------------------------------------------------------------------------------

// What is known about the value a wire slot holds, beyond its expression.  Wire slots are recycled: the facts of a slot's previous
// value end where an op overwrites it, while that op itself still reads its inputs' facts — so gen_ops takes a snapshot() before each op
// (what the op reads: `in`) and overwrite()s the op's output slots in the live set (what it writes: `of`).
struct WireFacts {
    // the tracks the value is a pure function of (with launch / per-voice constants): outputs of the stateless arithmetic modules fed
    // by such values.  Absent: the value has a history (an oscillator, a filter, an envelope, a delay ...).
    std::map<int, std::set<int>> pure;
    std::map<int, std::string> bounded;  // the wave-uniform condition under which the value is finite and small
    std::map<int, std::string> quiet;    // the expression of the value where that is one constant for a whole quiet group
    std::map<int, std::string> env;      // the envelope (its variables' prefix) whose quiet form produced it: a VCA behind it decides `cv > 0` per group
    WireFacts snapshot() const { return *this; }
    void overwrite(int slot)
    {
        pure.erase(slot);
        bounded.erase(slot);
        quiet.erase(slot);
        env.erase(slot);
    }
};

struct Gen {
    const FlatProgram& P;
    const GenKnobs& knobs;
    int out_mode;  // 1 frames, 2 mix, 3 both, 4 neither (the render only advances the voice state)
    std::ostringstream lds_rings, pro, tile_begin, body, tile_end, epi;
    bool needs_sync = false;     // LDS arrays filled in the prologue are read by other lanes
    int want_waves = 0;          // waves per SIMD the render has for this kernel (0: unknown) — what LDS beyond the mix tile it may spend
    int smp_lds_bytes = 0;       // LDS the sample players of this kernel have taken for staged waves so far (gen_sample)
    bool lds_tables = false;     // the pow tables of NonLinear / the sample player are in LDS (declared once per function)
    bool uses_ring_pos = false;  // some ring is addressed by the running position (n0 + t) mod buffer_size
    std::map<int, std::string> slot;  // wire slot -> the expression that currently holds it
    std::vector<int> tracks_used;
    // further per-sample values that are fetched a group of samples ahead and handed to the sample function as arguments:
    // (name, expression in terms of the sample index `i`)
    std::vector<std::pair<std::string, std::string>> sample_args;
    // Wave-uniform conditions the sample loop is versioned on: when all of them hold (the common case) a copy of the loop runs in
    // which each is a constant — (condition, the declaration that shadows it inside that copy).  The other copy keeps every arm.
    std::vector<std::pair<std::string, std::string>> fast_conds;
    WireFacts of, in_facts;  // per wire slot: as the ops so far leave it / as the op being generated reads it (gen_ops)
    bool pure_deps(int s, std::set<int>& deps)
    {
        if (s < 0) return true;  // an unconnected input: the constant 0.0
        if (s >= kTrackSlot) {
            deps.insert(s - kTrackSlot);
            return true;
        }
        const auto it = in_facts.pure.find(s);
        if (it == in_facts.pure.end()) return false;
        deps.insert(it->second.begin(), it->second.end());
        return true;
    }
    // Quiet groups (modules.hip.h, cosc_quiet_init): event machines — a gate LFO, the envelope behind it — ask once per group of kQuietGroup
    // samples whether any lane can have an event within the group; a group without one runs a second copy of the sample function in which
    // their per-sample questions are gone (`kQuiet`).  group_begin: evaluated at the start of every group (declares the per-group values);
    // quiet_lane: the per-lane conditions, all of which must hold in every lane; group_end_quiet: after a quiet group's samples.
    // Where a value is one constant for a whole quiet group, and which envelope's quiet form produced it: WireFacts::quiet / env.
    std::ostringstream group_decl, group_begin, group_end_quiet;  // (group_decl: per-group values the sample function reads, declared ahead of it)
    std::vector<std::string> quiet_lane;
    // A group that is not quiet as a whole takes the literal per-sample copy (with the modules' cold arms) for all of its samples, unrolled
    // (halving such a group instead was measured and not taken: notes/r29.md).  `kLen` / `kLi` in the per-group texts: the group's length
    // and its index into the per-length guards, constants of the kernel's quiet_run (emit_quiet_groups).
    static std::string indent(const std::string& text, int by)
    {
        std::istringstream in(text);
        std::string line, out;
        while (std::getline(in, line)) out += std::string((size_t)by, ' ') + line + "\n";
        return out;
    }
    std::map<int, bool> ring_declared;
    bool needs_full_unroll = false;  // a ring prefetch array is indexed by the sample's position in the tile
    std::string err;

    bool is_ctl = false;      // a unit of the control program (one voice): its planes are tracks, written 32 samples per store
    // A control unit whose every module has a tile-wise form is evaluated ACROSS LANES: lane j holds sample j of the tile.  Stateless
    // modules (VCA, mixer, math, waveshaper) simply compute 32 samples with one instruction each; a constant-pitch oscillator runs its
    // two-instruction phase recurrence and evaluates the outputs per lane (cosc_tile); an envelope takes whole runs of samples between
    // the events that can end its segment (adsr_seg_tile).  One voice on one wave is a latency chain — ~14 cycles per dependent
    // instruction, ~40 per branch —, so the sample-by-sample form costs 35 ... 100 ns per sample and module (tools/unit_times.py).
    bool across_lanes = false;
    std::string uniq;         // prefix of this function's __shared__ arrays (static LDS names share the kernel's scope)

    // LDS tiles of 32 rows x 64 lanes (wave.hip.h: kMixTile floats).  Every wire-fed output plane owns one for the mix-down; an
    // exact-mode saw oscillator needs one for its tile-wise evaluation (modules.hip.h, XSaw) and borrows the tile of an output
    // op that comes LATER in the op list: within a sample its row is read (at the oscillator's position) before the plane's
    // sample overwrites it (at the output op's position), and the whole tile is written before the sample loop starts.
    std::map<int, int> tile_of_out;     // OUT op index -> tile (planes fed by a wire, when the mix-down is on)
    std::map<int, bool> out_tile_lent;  // ... already borrowed by an oscillator
    int n_tiles = 0;
    std::vector<std::string> shared_emits;  // the Emit objects of the planes that share the tile, in plane order
    int rows_per_plane = 0;             // > 0: the planes share tile 0, plane j (tile_of_out's numbering) owns rows [j, j + 1) * rows_per_plane

    // ---- what is known about a wire ahead of time (voice programs): for the oscillators' pitch inputs ----------------------------------
    // The hand-written FM pair proves, per wave and launch, that its oscillators' CVs are bounded — a sine through a constant gain —
    // and takes a sample loop without range reduction, with a one-instruction phase wrap and val folded into a per-launch scale
    // (fm_common.hip.h, fm_facts).  The generator derives the same for ANY program: a magnitude bound per wire as an expression in the
    // program's parameters (|sine| <= 1, |saw|, |square| <= 2, |lowpass| <= 1, products and sums through Math / VCA / mixer, a delayed
    // edge inherits its source's), and every oscillator whose CV has one is VERSIONED: the wave votes once per launch (bound classes,
    // phases in [0, 1), ring contents within their bound) and runs the copy of the sample loop compiled for its classes
    // (modules.hip.h, fm_class_flags) — or the literal forms when the vote fails.  A launch is proved as a whole or not at all.
    struct Fact {
        std::string bound;     // per-lane float expression over parameters: |value| <= bound all launch long, given the vote; "": unknown
        bool audio = false;    // changes from sample to sample (an oscillator, a filter, an envelope, noise ... somewhere upstream)
        std::set<int> oscs;    // oscillators (op indices) whose phase must be, and stay, in [0, 1) for the bound to hold
        std::set<int> rings;   // DELAY_RD ops whose stored values must be within their bound when the launch starts
        std::set<std::string> also;  // further per-lane conditions of the vote, ready-made (an envelope's increments are not negative ...)
    };
    std::vector<Fact> cv_fact;            // per op (OP_OSC): what is known about its CV input
    std::vector<Fact> rd_fact;            // per op (OP_DELAY_RD): what it hands on
    std::vector<int> fm_index;            // per op: which versioned oscillator it is (-1: none)
    std::vector<int> fm_ops;              // the versioned oscillators, in op order
    std::map<int, std::string> osc_pos, osc_delta;  // per oscillator op: the expressions of its phase / its constant increment ("" = host-proved)
    std::map<int, std::string> ring_check_of;       // per local ring (first state row): the same, as its declaration spells the ring
    std::map<int, std::string> ring_check;          // per DELAY_RD op: "every stored value is within `B`" with B to be substituted for @
    static Fact fact_join(const Fact& a, const Fact& b, const std::string& bound)
    {
        Fact f;
        f.bound = (a.bound.empty() || b.bound.empty()) ? "" : bound;
        f.audio = a.audio || b.audio;
        f.oscs = a.oscs;
        f.oscs.insert(b.oscs.begin(), b.oscs.end());
        f.rings = a.rings;
        f.rings.insert(b.rings.begin(), b.rings.end());
        f.also = a.also;
        f.also.insert(b.also.begin(), b.also.end());
        return f;
    }
    // which op wrote the value wire slot `s` holds when op `at` reads it, and through which port
    bool producer_of(int s, int at, int& op_out, int& port_out) const
    {
        for (int k = at - 1; k >= 0; k--)
            for (int p = 0; p < kMaxOut; p++)
                if (P.ops[(size_t)k].out_slot[p] == s) {
                    op_out = k;
                    port_out = p;
                    return true;
                }
        return false;
    }
    // What a DELAY_RD hands on.  What the ring holds was written by the matching DELAY_WR — of an op further down the list, usually: its
    // value's own bound is what counts (an oscillator's port, a filter's lowpass / bandpass, noise), given that the stored values respect
    // it too when the launch starts.
    // distrusted: oscillators a delayed edge took for bounded although their own CV is not; assumed: those taken for bounded in this pass
    Fact ring_fact(int k, bool bounds, const std::set<int>& distrusted, std::set<int>& assumed) const
    {
        const DevOp& op = P.ops[(size_t)k];
        const int n = (int)P.ops.size();
        Fact f;
        f.audio = true;
        const bool global = (op.flags & DELAY_RING_GLOBAL) != 0;
        if (!bounds || global || P.hdr.buffer_size > 16) return f;
        for (int w = 0; w < n; w++) {
            const DevOp& wr = P.ops[(size_t)w];
            if (wr.kind != OP_DELAY_WR || wr.aux != op.aux || ((wr.flags & DELAY_RING_GLOBAL) != 0) != global) continue;
            int pk = -1, pp = -1;
            if (!producer_of(wr.in_slot[0], w, pk, pp)) break;
            const DevOp& src = P.ops[(size_t)pk];
            if (src.kind == OP_OSC && !(src.flags & OSC_EXACT) && pp < 3 && !distrusted.count(pk)) {
                f.bound = pp == 0 ? "1.0f" : "2.0f";
                f.oscs.insert(pk);
                if (src.flags & OSC_HAS_CV) assumed.insert(pk);
            } else if (src.kind == OP_VCF && pp < 2) {
                f.bound = pp == 0 ? "1.0f" : "6.0f";
            } else if (src.kind == OP_NOISE) {
                f.bound = "1.0f";
            }
            break;
        }
        if (!f.bound.empty()) f.rings.insert(k);
        return f;
    }
    // the facts of op k's outputs, given those of its inputs (and cv_fact / rd_fact of the op itself, for the generator)
    void op_facts(int k, bool bounds, const std::map<int, Fact>& cur, const std::set<int>& distrusted, std::set<int>& assumed, Fact outs[kMaxOut])
    {
        const DevOp& op = P.ops[(size_t)k];
        const std::string m = "m" + std::to_string(k);
        auto get = [&](int sl) -> Fact {
            Fact f;
            if (sl < 0) f.bound = "0.0f";  // an unconnected input reads 0.0
            const auto it = cur.find(sl);  // (a control track is no op's output: anything — and constant for long stretches more often than not)
            return it == cur.end() ? f : it->second;
        };
        auto source = [&](const char* b) {  // a value with a history of its own
            Fact f;
            f.bound = bounds ? b : "";
            f.audio = true;
            return f;
        };
        switch (op.kind) {
        case OP_OSC: {
            const Fact cv = (op.flags & OSC_HAS_CV) ? get(op.in_slot[0]) : Fact{};
            cv_fact[(size_t)k] = cv;
            const bool phase_ok = !(op.flags & OSC_EXACT) && (!(op.flags & OSC_HAS_CV) || !cv.bound.empty());
            for (int p = 0; p < 3; p++) {
                outs[p] = source(phase_ok ? (p == 0 ? "1.0f" : "2.0f") : "");
                outs[p].oscs = cv.oscs;
                outs[p].rings = cv.rings;
                outs[p].also = cv.also;
                outs[p].oscs.insert(k);
            }
            break;
        }
        case OP_VCF: {
            const Fact a = get(op.in_slot[0]);
            outs[0] = source("1.0f");                                                 // b4, clamped to [-1, 1]
            outs[1] = source("6.0f");                                                 // 3 (b3 - b4)
            outs[2] = fact_join(a, source("1.0f"), "(" + a.bound + " + 6.0f)");        // (in - q b4) - b4, q <= 3.8
            outs[2].audio = true;
            break;
        }
        case OP_NOISE: outs[0] = source("1.0f"); break;
        case OP_ADSR:  // the hull of {0, 1, s_val, r_val, from_a_val} (modules.hip.h, adsr_bound), given sane time constants
            outs[0] = source(("adsr_bound(" + m + ", " + m + "_k)").c_str());
            if (bounds) outs[0].also.insert("adsr_tame(" + m + ", " + m + "_k)");
            break;
        case OP_NONLIN:
        case OP_SAMPLE: outs[0] = source(""); break;
        case OP_GRIDSEQ:
        case OP_PATSEQ: break;  // stepwise values of any size
        case OP_MATH: {
            const Fact a = (op.flags & MATH_HAS_IN1) ? get(op.in_slot[0]) : get(-1);
            Fact b;
            if (op.flags & MATH_HAS_IN2)
                b = get(op.in_slot[1]);
            else
                b.bound = "__builtin_fabsf(" + m + "_c)";
            const bool mul = ((op.flags >> MATH_OP_SHIFT) & 3u) == SRACK_MATH_MULTIPLY;
            outs[0] = fact_join(a, b, "(" + a.bound + (mul ? " * " : " + ") + b.bound + ")");
            break;
        }
        case OP_VCA: {
            if ((op.flags & (VCA_HAS_AUDIO | VCA_HAS_CV)) != (VCA_HAS_AUDIO | VCA_HAS_CV)) {
                outs[0] = get(-1);
                break;
            }
            const Fact a = get(op.in_slot[0]), b = get(op.in_slot[1]);
            outs[0] = fact_join(a, b, "(" + a.bound + " * " + b.bound + ")");
            break;
        }
        case OP_MIX: {
            Fact acc = get(-1);
            for (int j = 0; j < 4; j++) {
                if (!(op.flags & (1u << j))) continue;
                const Fact x = get(op.in_slot[j]);
                acc = fact_join(acc, x, "(" + acc.bound + " + " + x.bound + " * __builtin_fabsf(" + m + "_g[" + std::to_string(j) + "]))");
            }
            outs[0] = acc;
            break;
        }
        case OP_DELAY_RD:
            rd_fact[(size_t)k] = ring_fact(k, bounds, distrusted, assumed);
            outs[0] = rd_fact[(size_t)k];
            break;
        default: break;
        }
    }
    void analyze()
    {
        const int n = (int)P.ops.size();
        cv_fact.assign((size_t)n, Fact{});
        rd_fact.assign((size_t)n, Fact{});
        fm_index.assign((size_t)n, -1);
        fm_ops.clear();
        if (is_ctl) return;
        const bool bounds = !(P.render_flags & SRACK_RENDER_EXACT_OSC) && knobs.fm;
        std::set<int> distrusted;  // oscillators a delayed edge took for bounded although their own CV is not
        for (int iter = 0; iter <= n; iter++) {
            std::map<int, Fact> cur;
            std::set<int> assumed;
            for (int k = 0; k < n; k++) {
                Fact outs[kMaxOut];
                op_facts(k, bounds, cur, distrusted, assumed, outs);
                for (int p = 0; p < kMaxOut; p++)
                    if (P.ops[(size_t)k].out_slot[p] >= 0) cur[P.ops[(size_t)k].out_slot[p]] = outs[p];
            }
            bool changed = false;
            for (int k : assumed)
                if (cv_fact[(size_t)k].bound.empty() && !distrusted.count(k)) {
                    distrusted.insert(k);
                    changed = true;
                }
            if (!changed) break;
        }
        // a bound that rests on an oscillator with an unbounded CV of its own does not hold
        for (int k = 0; k < n; k++) {
            Fact& f = cv_fact[(size_t)k];
            for (int o : std::set<int>(f.oscs))
                if (o != k && (P.ops[(size_t)o].flags & OSC_HAS_CV) && cv_fact[(size_t)o].bound.empty()) f.bound.clear();
        }
        for (int k = 0; k < n && bounds; k++)
            if (P.ops[(size_t)k].kind == OP_OSC && (P.ops[(size_t)k].flags & OSC_HAS_CV) && (P.ops[(size_t)k].flags & OSC_CV_AUDIO_RATE) && !cv_fact[(size_t)k].bound.empty()) {  // (a CV that holds keeps the literal form: the reference's own increment per held value)
                fm_index[(size_t)k] = (int)fm_ops.size();
                fm_ops.push_back(k);
            }
        if (fm_ops.size() > 6) {  // (the copies of the sample loop multiply)
            for (int k : fm_ops) fm_index[(size_t)k] = -1;
            fm_ops.clear();
        }
    }
    // the classes a versioned oscillator may take, by how many of them share the loop's copies: {1, 2, 3} / {1, 3} / {1}
    int fm_classes() const { return fm_ops.size() <= 2 ? 3 : fm_ops.size() == 3 ? 2 : 1; }

    bool tile_wise(const DevOp& op) const
    {
        const uint32_t fl = op.flags;
        const uint32_t ports = fl & (OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW);
        switch (op.kind) {
        case OP_VCA:
        case OP_MIX:
        case OP_MATH:
        case OP_NONLIN:
        case OP_OUT: return true;
        case OP_ADSR: return (fl & ADSR_HAS_GATE) != 0;
        case OP_OSC:  // constant pitch, no sync, one live port, increment below 1/4 (host-proved)
            return ports && !(ports & (ports - 1)) && ((fl & OSC_CONST_FAST) || ((fl & OSC_EXACT) && (fl & OSC_CONST_SMALL)));
        default: return false;
        }
    }
    Gen(const FlatProgram& p, const GenKnobs& kn, int om, bool ctl = false, const std::string& u = "") : P(p), knobs(kn), out_mode(om), is_ctl(ctl), uniq(u)
    {
        if (is_ctl && knobs.across_lanes) {
            across_lanes = true;
            for (const DevOp& op : P.ops) across_lanes = across_lanes && tile_wise(op);
        }
        if (!is_ctl && (out_mode & 2))
            for (int k = 0; k < (int)P.ops.size(); k++)
                if (P.ops[(size_t)k].kind == OP_OUT && P.ops[(size_t)k].in_slot[0] < kTrackSlot) tile_of_out[k] = n_tiles++;
        // default mode (no tile-wise exact saw borrows a plane's tile): two or more planes share one tile, 32 / P' rows each (wave.hip.h)
        // (who borrows: gen_osc's two tile-wise exact saws — an exact oscillator whose only live port is the saw, at a constant pitch or with a CV and no sync; any other exact oscillator,
        // e.g. in a patch the flattener turned exact because a loop runs through a pitch, leaves the tiles alone)
        bool borrower = false;
        for (const DevOp& op : P.ops)
            borrower = borrower || (op.kind == OP_OSC && (op.flags & OSC_EXACT) && (op.flags & (OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW)) == OSC_OUT_SAW &&
                                    ((op.flags & OSC_CONST_SMALL) || (op.flags & (OSC_HAS_CV | OSC_HAS_SYNC | OSC_AA)) == (OSC_HAS_CV | OSC_AA)));  // (a superset of gen_osc's two cases)
        if (n_tiles >= 2 && !borrower && !knobs.tile_per_plane) {
            rows_per_plane = n_tiles <= 2 ? 16 : 8;  // (jit_supported: at most four distinct planes)
            n_tiles = 1;
        }
        analyze();
    }
    int borrow_tile(int after_op)
    {
        if (rows_per_plane > 0) return n_tiles++;  // (the planes share tile 0 row-wise: nothing to lend — cannot happen, the constructor looks for borrowers first)
        for (auto& kv : tile_of_out)
            if (kv.first > after_op && !out_tile_lent[kv.first]) {
                out_tile_lent[kv.first] = true;
                return kv.second;
            }
        return n_tiles++;
    }

    static std::string hex(uint32_t v)
    {
        char b[16];
        std::snprintf(b, sizeof b, "0x%xu", v);
        return b;
    }
    std::string in(int s)
    {
        if (s < 0) return "zero_in";  // an unconnected input: 0.0, opaque to the optimiser (modules.hip.h, zero_f32)
        if (s >= kTrackSlot) {
            const int k = s - kTrackSlot;
            if (std::find(tracks_used.begin(), tracks_used.end(), k) == tracks_used.end()) tracks_used.push_back(k);
            // A control unit is ONE wave on a latency chain: a scalar load per sample would put ~200 cycles of memory latency on
            // every step.  Its input tracks are fetched a 32-sample tile ahead, lane j holding sample j, and read with v_readlane.
            if (is_ctl && across_lanes) return "trk" + std::to_string(k) + "_t";  // lane j holds sample j of the tile
            if (is_ctl) return "readlane_f32(trk" + std::to_string(k) + "_t, i)";
            // A voice wave reads the track through the scalar unit (it is wave-uniform), a group of samples per load: the sample
            // function receives its value as an argument (emit_function_body).
            return "tk" + std::to_string(k);
        }
        auto it = slot.find(s);
        if (it == slot.end()) {
            err = "wire slot read before it was written";
            return "0.0f";
        }
        return it->second;
    }
    std::string par(int k, int j)
    {
        const DevOp& op = P.ops[(size_t)k];
        if (op.par_row[j] >= 0) return "rowf(" + std::to_string(op.par_row[j]) + ")";
        return "a.ops[" + std::to_string(k) + "].par_val[" + std::to_string(j) + "]";
    }

    // an oscillator's three state rows as the launch leaves them: the f64 phase in two, the sync input's last level in the third
    void put_phase(int sr, const std::string& pos, const std::string& sync)
    {
        epi << "        put(" << sr << ", f64_lo(" << pos << ")); put(" << sr + 1 << ", f64_hi(" << pos << ")); put(" << sr + 2 << ", " << sync << ");\n";
    }

    void gen_osc(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        const uint32_t fl = op.flags;
        const uint32_t ports = fl & (OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW);
        const int sr = op.state_row;
        const std::string pos = "make_f64(row(" + std::to_string(sr) + "), row(" + std::to_string(sr + 1) + "))";
        const std::string delta = op.delta_row >= 0 ? "make_f64(row(" + std::to_string(op.delta_row) + "), row(" + std::to_string(op.delta_row + 1) + "))"
                                                     : "a.ops[" + std::to_string(k) + "].delta";
        const int port_index = (fl & OSC_OUT_SAW) ? 2 : (fl & OSC_OUT_SQUARE) ? 1 : 0;
        const bool one_port = ports && !(ports & (ports - 1));
        const bool exact = (fl & OSC_EXACT) != 0;
        if (across_lanes) {  // (tile_wise(): constant pitch, one port) the phase recurrence per sample, the outputs per lane
            pro << "    COsc " << m << ";\n    cosc_init(" << m << ", " << pos << ", " << delta << ");\n";
            body << "        const float " << m << "_y = cosc_tile<" << (exact ? "true" : "false") << ">(" << hex(fl & ~(OSC_CONST_FAST | OSC_CONST_SMALL)) << ", " << m << ", n);\n";
            slot[op.out_slot[port_index]] = m + "_y";
            put_phase(sr, m + ".pos", "0u");
            return;
        }
        if ((fl & OSC_CONST_FAST) && (fl & OSC_FIXED_PHASE)) {  // ... its saw with the phase in 2^-64 fixed point (host-set: nothing integrates or thresholds the value)
            const std::string dlo = op.delta_row >= 0 ? "row(" + std::to_string(op.delta_row) + ")" : "(uint32_t)(uint64_t)__double_as_longlong(a.ops[" + std::to_string(k) + "].delta)";
            const std::string dhi = op.delta_row >= 0 ? "row(" + std::to_string(op.delta_row + 1) + ")" : "(uint32_t)((uint64_t)__double_as_longlong(a.ops[" + std::to_string(k) + "].delta) >> 32)";
            osc_pos[k] = "0.0";   // (a fixed-point phase is in [0, 1) by construction)
            osc_delta[k] = "";
            pro << "    FOsc " << m << ";\n    fosc_init(" << m << ", row(" << sr << "), row(" << sr + 1 << "), " << dlo << ", " << dhi << ");\n";
            body << "        const float " << m << "_y = fosc_saw(" << m << ");\n";
            slot[op.out_slot[2]] = m + "_y";
            epi << "        put(" << sr << ", " << m << ".lo); put(" << sr + 1 << ", " << m << ".hi); put(" << sr + 2 << ", 0u);\n";
            return;
        }
        if (fl & OSC_CONST_FAST) {  // no CV, no sync, one live port, delta < 0.25 everywhere: the carried-phase oscillator
            osc_pos[k] = m + ".pos";
            osc_delta[k] = "";  // host-proved: 0 <= delta < 1/4
            pro << "    COsc " << m << ";\n    cosc_init(" << m << ", " << pos << ", " << delta << ");\n";
            if (ports == OSC_OUT_SQUARE && !is_ctl && knobs.quiet) {
                // a square at a constant pitch is a gate source more often than not: outside its PolyBLEP windows it is one level for a whole group
                pro << "    COscQuiet " << m << "_q[1];\n    cosc_quiet_init(" << m << ", " << m << "_q[0], 8);\n";
                group_decl << "        float " << m << "_lv = 0.0f;\n";
                group_begin << "                " << m << "_lv = cosc_square_level(" << m << ");\n";
                quiet_lane.push_back("cosc_square_quiet(" + m + ", " + m + "_q[kLi])");
                body << "        float " << m << "_y;\n        if constexpr (kQuiet) {\n            " << m << "_y = " << m << "_lv;\n            cosc_quiet_step(" << m
                     << ");\n        } else {\n            " << m << "_y = cosc_step<" << hex(ports) << ">(" << m << ");\n        }\n";
                of.quiet[op.out_slot[port_index]] = m + "_lv";
            } else {
                body << "        const float " << m << "_y = cosc_step<" << hex(ports) << ">(" << m << ");\n";
            }
            slot[op.out_slot[port_index]] = m + "_y";
            put_phase(sr, m + ".pos", "0u");
            return;
        }
        if (exact && (fl & OSC_CONST_SMALL) && one_port && (ports == OSC_OUT_SQUARE || (ports == OSC_OUT_SAW && is_ctl))) {
            // exact mode, constant pitch, where PolyBLEP windows are rare (a square is an LFO / clock more often than not; a control unit
            // is one voice): the reference's formulas only for the samples with a lane inside a window (modules.hip.h, cosc_exact_step)
            pro << "    COsc " << m << ";\n    cosc_init(" << m << ", " << pos << ", " << delta << ");\n";
            body << "        const float " << m << "_y = cosc_exact_step<" << hex(ports) << ">(" << m << ");\n";
            slot[op.out_slot[port_index]] = m + "_y";
            put_phase(sr, m + ".pos", "0u");
            return;
        }
        pro << "    OscConst " << m << "_k;\n    " << m << "_k.sr = a.ops[" << k << "].sample_rate;\n    " << m << "_k.val = (double)" << par(k, OSC_P_VAL) << ";\n";
        if (!(fl & OSC_HAS_CV))
            pro << "    " << m << "_k.delta = " << delta << ";\n    " << m << "_k.inv_dt = inv_dt_f32(" << m << "_k.delta);\n";
        else
            pro << "    " << m << "_k.delta = 0.0;\n    " << m << "_k.inv_dt = 0.0f;\n";
        if (!exact && (fl & (OSC_HAS_CV | OSC_CV_STEPWISE | OSC_HAS_SYNC | OSC_AA | OSC_EXACT_BLEP)) == (OSC_HAS_CV | OSC_CV_STEPWISE | OSC_AA) && one_port) {
            osc_pos[k] = m + ".o.pos";
            pro << "    StepOsc " << m << ";\n    steposc_init(" << m << ", " << pos << ");\n";
            body << "        const float " << m << "_y = steposc_step<" << hex(ports) << ">(" << m << ", " << m << "_k, " << in(op.in_slot[0]) << ");\n";
            slot[op.out_slot[port_index]] = m + "_y";
            put_phase(sr, m + ".o.pos", "0u");
            return;
        }
        pro << "    OscRegs " << m << ";\n    " << m << ".pos = " << pos << ";\n    " << m << ".sync_last = row(" << sr + 2 << ") != 0;\n";
        if (exact && !is_ctl && (fl & OSC_CONST_SMALL) && ports == OSC_OUT_SAW) {
            // Exact mode, constant pitch, saw: a tile at a time (windowless values, then each lane repairs its own PolyBLEP rows with
            // the reference's f64 division) instead of paying for the division whenever ANY lane of the wave is inside a window.
            // Its preconditions are checked once per launch; a wave that fails them takes the literal per-sample form.
            const int tile = borrow_tile(k);
            pro << "    XSaw " << m << "_x;\n    const bool " << m << "_xs = xsaw_usable(" << m << ".pos, " << m << "_k.delta);\n";
            pro << "    if (" << m << "_xs) xsaw_init(" << m << "_x, " << m << ".pos, " << m << "_k.delta);\n";
            pro << "    float* const " << m << "_xt = mix_tile + " << tile << " * kMixTile + lane;\n";
            tile_begin << "        if (" << m << "_xs) xsaw_tile(" << m << "_x, " << m << "_xt, kMixPitch, n);\n";
            // the tile's row of sample i, read ahead of the group of samples it belongs to (before the plane that lent the tile overwrites it)
            sample_args.emplace_back(m + "_xr", m + "_xs ? " + m + "_xt[(i) * kMixPitch] : 0.0f");
            of.bounded[op.out_slot[2]] = m + "_xs";  // XSaw's preconditions bound the saw by 2
            fast_conds.emplace_back(m + "_xs", "constexpr bool " + m + "_xs = true;");
            body << "        float " << m << "_y2;\n        if (" << m << "_xs) {\n            " << m << "_y2 = " << m << "_xr;\n        } else {\n";
            body << "            float " << m << "_y0 = 0.0f, " << m << "_y1 = 0.0f;\n            " << m << "_y2 = 0.0f;\n";
            body << "            osc_step(" << hex(fl) << ", " << m << ", " << m << "_k, zero_in, zero_in, " << m << "_y0, " << m << "_y1, " << m << "_y2);\n        }\n";
            slot[op.out_slot[2]] = m + "_y2";
            epi << "        if (" << m << "_xs) { " << m << ".pos = " << m << "_x.pos; " << m << ".sync_last = false; }\n";
            put_phase(sr, m + ".pos", m + ".sync_last ? 1u : 0u");
            return;
        }
        std::set<int> cv_tracks;
        if (exact && !is_ctl && (fl & (OSC_HAS_CV | OSC_HAS_SYNC | OSC_AA)) == (OSC_HAS_CV | OSC_AA) && ports == OSC_OUT_SAW && pure_deps(op.in_slot[0], cv_tracks)) {
            // Exact mode, saw, a pitch that is a pure function of control tracks (a sequencer's note, transposed per voice): wherever those
            // tracks hold one value for a whole tile — decided at the tile's first sample, when the CV of that sample is known — the
            // increment is the one of that CV and the tile is written by the tile-wise saw (XSaw), as for a constant pitch.  Other tiles
            // (a note change inside, a glide, the tail of a launch) take the literal per-sample form; the phase is common to both.
            const int tile = borrow_tile(k);
            const std::string cv = in(op.in_slot[0]);
            pro << "    XSaw " << m << "_x;\n    bool " << m << "_flat = false;\n    float* const " << m << "_xt = mix_tile + " << tile << " * kMixTile + lane;\n";
            body << "        const float " << m << "_cv = " << cv << ";\n";
            body << "        if (i == 0) {\n            " << m << "_flat = n == kMixRows";
            for (int tk : cv_tracks) body << " && track_flat(trk" << tk << "_v + t0, lane)";
            body << ";\n            if (" << m << "_flat) {\n";
            body << "                if (__builtin_amdgcn_ballot_w64(" << m << "_cv != " << m << ".seen_cv) != 0) {\n";
            body << "                    " << m << ".seen_delta = 440.0 * exp2_libm((double)" << m << "_cv + " << m << "_k.val) / " << m << "_k.sr;  // osc_step's own, exact flavour\n";
            body << "                    " << m << ".seen_cv = " << m << "_cv;\n                }\n";
            body << "                " << m << "_flat = xsaw_usable(" << m << ".pos, " << m << ".seen_delta);\n";
            body << "                if (" << m << "_flat) {\n                    xsaw_init(" << m << "_x, " << m << ".pos, " << m << ".seen_delta);\n";
            body << "                    xsaw_tile(" << m << "_x, " << m << "_xt, kMixPitch, kMixRows);\n";
            body << "                    " << m << ".pos = " << m << "_x.pos;\n                    " << m << ".sync_last = false;\n                }\n            }\n        }\n";
            body << "        float " << m << "_y2;\n        if (" << m << "_flat) {\n            " << m << "_y2 = " << m << "_xt[i * kMixPitch];\n        } else {\n";
            body << "            float " << m << "_y0 = 0.0f, " << m << "_y1 = 0.0f;\n            " << m << "_y2 = 0.0f;\n";
            body << "            osc_step(" << hex(fl) << ", " << m << ", " << m << "_k, " << m << "_cv, zero_in, " << m << "_y0, " << m << "_y1, " << m << "_y2);\n        }\n";
            slot[op.out_slot[2]] = m + "_y2";
            of.bounded[op.out_slot[2]] = m + "_flat";  // (per tile, not per launch: a filter behind it tests a scalar instead of its input)
            put_phase(sr, m + ".pos", m + ".sync_last ? 1u : 0u");
            return;
        }
        const std::string cv = in(op.in_slot[0]), sync = in(op.in_slot[1]);
        osc_pos[k] = m + ".pos";
        osc_delta[k] = (fl & OSC_HAS_CV) ? "" : m + "_k.delta";
        // a CV that derives from an oscillator, a filter, an envelope ... changes every sample: no point in comparing it with the last one
        std::string fx = hex(fl);  // (OSC_CV_AUDIO_RATE is the flattener's: a CV that sweeps, flatten.cpp `sweeps`; an envelope's or a sequencer's holds)
        if (!is_ctl && fm_index[(size_t)k] >= 0) {  // a bounded CV: the flags of the class its wave voted for (analyze)
            fx = "(" + fx + " | kFm" + std::to_string(fm_index[(size_t)k]) + ")";
            pro << "    " << m << "_k.scale = (440.0 / " << m << "_k.sr) * exp2(" << m << "_k.val);  // OSC_VAL_FOLDED: the increment is scale * 2^cv\n";
        }
        body << "        float " << m << "_y0 = 0.0f, " << m << "_y1 = 0.0f, " << m << "_y2 = 0.0f;\n";
        body << "        osc_step(" << fx << ", " << m << ", " << m << "_k, " << cv << ", " << sync << ", " << m << "_y0, " << m << "_y1, " << m << "_y2);\n";
        for (int p = 0; p < 3; p++)
            if (op.out_slot[p] >= 0) slot[op.out_slot[p]] = m + "_y" + std::to_string(p);
        put_phase(sr, m + ".pos", m + ".sync_last ? 1u : 0u");
    }

    void gen_vcf(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        const int s0 = op.state_row;
        const bool fast = !(P.render_flags & SRACK_RENDER_EXACT_OSC) && !(op.flags & VCF_LITERAL);
        const char* F = fast ? "true" : "false";
        pro << "    VcfRegs " << m << ";\n";
        const char* names[10] = {"f", "p", "q", "b0", "b1", "b2", "b3", "b4", "freq", "res"};
        for (int j = 0; j < 10; j++) pro << "    " << m << "." << names[j] << " = rowf(" << s0 + j << ");\n";
        pro << "    const float " << m << "_freq = " << par(k, VCF_P_FREQ) << ", " << m << "_exp = " << par(k, VCF_P_EXP) << ", " << m << "_res = vcf_resonance("
            << par(k, VCF_P_RES) << ");\n";
        pro << "    bool " << m << "_fin = " << (fast ? "true" : "vcf_nan_free(" + m + ")") << ";\n";
        const std::string audio = in(op.in_slot[0]);
        if (op.flags & VCF_HAS_CV) {  // `res` is a parameter: settled before the first sample, the loop compares the frequency only
            pro << "    if (a.T > 0) vcf_res_settle(" << m << ", " << m << "_res);\n";
            body << "        vcf_coeffs_freq<" << F << ">(" << m << ", " << (fast ? "vcf_frequency_med3(" : "vcf_frequency(") << m << "_freq, " << in(op.in_slot[1]) << ", "
                 << m << "_exp), " << m << "_res);\n";
        } else  // constant cutoff: the "did (frequency, res) change" check can only fire on the first sample
            pro << "    if (a.T > 0) vcf_coeffs<" << F << ">(" << m << ", vcf_frequency(" << m << "_freq, 0.0f, " << m << "_exp), " << m << "_res);\n";
        body << "        float " << m << "_lp, " << m << "_bp, " << m << "_hp;\n";
        const auto bounded = in_facts.bounded.find(op.in_slot[0]);
        if (!fast && bounded != in_facts.bounded.end()) fast_conds.emplace_back(m + "_fin", "bool " + m + "_fin = true;");
        if (!fast && bounded != in_facts.bounded.end())  // no per-sample look at the input's magnitude
            body << "        vcf_run_bounded(" << m << ", " << m << "_fin, " << bounded->second << ", " << audio << ", " << m << "_lp, " << m << "_bp, " << m << "_hp);\n";
        else
            body << "        vcf_run<" << F << ">(" << m << ", " << m << "_fin, " << audio << ", " << m << "_lp, " << m << "_bp, " << m << "_hp);\n";
        const char* outs[3] = {"_lp", "_bp", "_hp"};
        for (int p = 0; p < 3; p++)
            if (op.out_slot[p] >= 0) slot[op.out_slot[p]] = m + outs[p];
        epi << "       ";
        for (int j = 0; j < 10; j++) epi << " put(" << s0 + j << ", __float_as_uint(" << m << "." << names[j] << "));";
        epi << "\n";
    }

    void gen_adsr(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        const int sr = op.state_row;
        pro << "    AdsrRegs " << m << ";\n";
        pro << "    " << m << ".phase = rowf(" << sr + ADSR_S_PHASE << "); " << m << ".mode = (int)row(" << sr + ADSR_S_MODE << "); " << m << ".r_val = rowf("
            << sr + ADSR_S_R_VAL << "); " << m << ".from_a_val = rowf(" << sr + ADSR_S_FROM_A << "); " << m << ".gate_last = row(" << sr + ADSR_S_GATE_LAST << ") != 0;\n";
        pro << "    const AdsrConst " << m << "_k = adsr_consts(" << par(k, ADSR_P_A) << ", " << par(k, ADSR_P_D) << ", " << par(k, ADSR_P_S) << ", " << par(k, ADSR_P_R)
            << ", " << par(k, ADSR_P_SR) << ");\n";
        if (op.flags & ADSR_HAS_GATE) {  // the segmented form: adsr.rs's own operations between mode changes (modules.hip.h)
            pro << "    AdsrSeg " << m << "_g;\n    adsr_seg_enter(" << m << ", " << m << "_k, " << m << "_g);\n";
            const auto lv = in_facts.quiet.find(op.in_slot[0]);
            const char* seg_step = "adsr_seg_step";
            if (across_lanes) {
                body << "        const float " << m << "_y = adsr_seg_tile(" << m << ", " << m << "_k, " << m << "_g, " << in(op.in_slot[0]) << ", n);\n";
            } else if (!is_ctl && lv != in_facts.quiet.end()) {
                // the gate is one level for a whole quiet group: the envelope asks its questions once per group (modules.hip.h, adsr_seg_quiet)
                group_begin << "                uint64_t " << m << "_qh;\n                const bool " << m << "_ql = adsr_seg_quiet(" << m << ", " << m << "_g, " << lv->second << ", "
                            << m << "_qh, kLen);\n";
                quiet_lane.push_back(m + "_ql");
                group_end_quiet << "                    " << m << "_g.last = " << m << "_qh;\n";
                of.env[op.out_slot[0]] = m;
                body << "        float " << m << "_y;\n        if constexpr (kQuiet) {\n            " << m << "_y = adsr_seg_quiet_step(" << m << ", " << m
                     << "_g);\n        } else {\n            " << m << "_y = " << seg_step << "(" << m << ", " << m << "_k, " << m << "_g, " << in(op.in_slot[0]) << ");\n        }\n";
            } else {
                body << "        const float " << m << "_y = " << seg_step << "(" << m << ", " << m << "_k, " << m << "_g, " << in(op.in_slot[0]) << ");\n";
            }
            epi << "        adsr_seg_flush(" << m << ", " << m << "_g);\n";
        } else {
            body << "        const float " << m << "_y = adsr_step(" << hex(op.flags) << ", " << m << ", " << m << "_k, 0.0f);\n";
        }
        slot[op.out_slot[0]] = m + "_y";
        epi << "        put(" << sr + ADSR_S_PHASE << ", __float_as_uint(" << m << ".phase)); put(" << sr + ADSR_S_MODE << ", (uint32_t)" << m << ".mode); put("
            << sr + ADSR_S_R_VAL << ", __float_as_uint(" << m << ".r_val)); put(" << sr + ADSR_S_FROM_A << ", __float_as_uint(" << m << ".from_a_val)); put("
            << sr + ADSR_S_GATE_LAST << ", " << m << ".gate_last ? 1u : 0u);\n";
    }

    void gen_simple(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        switch (op.kind) {
        case OP_VCA: {
            pro << "    const bool " << m << "_neg = " << par(k, VCA_P_NEG) << " != 0.0f;\n";
            const auto env = in_facts.env.find(op.in_slot[1]);
            if (!is_ctl && env != in_facts.env.end() && (op.flags & (VCA_HAS_AUDIO | VCA_HAS_CV)) == (VCA_HAS_AUDIO | VCA_HAS_CV)) {
                // the CV is an envelope in its quiet form: `cv > 0.0` has one answer per lane and group (modules.hip.h, adsr_seg_open)
                const std::string& e = env->second;
                group_decl << "        bool " << m << "_open = false;\n";
                group_begin << "                bool " << m << "_dec;\n                " << m << "_open = adsr_seg_open(" << e << ", " << e << "_g, " << m << "_dec) || " << m
                            << "_neg;\n";
                quiet_lane.push_back("(" + m + "_dec || " + m + "_neg)");
                body << "        float " << m << "_y;\n        if constexpr (kQuiet) {\n            " << m << "_y = vca_step_decided(" << m << "_open, " << in(op.in_slot[0]) << ", "
                     << in(op.in_slot[1]) << ");\n        } else {\n            " << m << "_y = vca_step(" << hex(op.flags) << ", " << m << "_neg, " << in(op.in_slot[0]) << ", "
                     << in(op.in_slot[1]) << ");\n        }\n";
            } else {
                body << "        const float " << m << "_y = " << (!is_ctl && op.in_slot[1] >= kTrackSlot ? "vca_step_uniform(" : "vca_step(") << hex(op.flags) << ", " << m
                     << "_neg, " << in(op.in_slot[0]) << ", " << in(op.in_slot[1]) << ");\n";
            }
            break;
        }
        case OP_MIX:
            pro << "    const float " << m << "_g[4] = {" << par(k, MIX_P_GAIN0) << ", " << par(k, MIX_P_GAIN0 + 1) << ", " << par(k, MIX_P_GAIN0 + 2) << ", "
                << par(k, MIX_P_GAIN0 + 3) << "};\n";
            body << "        const float " << m << "_x[4] = {" << in(op.in_slot[0]) << ", " << in(op.in_slot[1]) << ", " << in(op.in_slot[2]) << ", " << in(op.in_slot[3]) << "};\n";
            body << "        const float " << m << "_y = mixer_step(" << hex(op.flags) << ", " << m << "_x, " << m << "_g);\n";
            break;
        case OP_MATH:
            pro << "    const float " << m << "_c = " << par(k, MATH_P_CONST) << ";\n";
            body << "        const float " << m << "_y = math_step(" << hex(op.flags) << ", " << in(op.in_slot[0]) << ", " << in(op.in_slot[1]) << ", " << m << "_c);\n";
            break;
        case OP_NONLIN:
            pro << "    const float " << m << "_c = " << par(k, NONLIN_P_CONST) << ";\n";
            want_lds_tables();
            body << "        const float " << m << "_y = nonlin_step(" << hex(op.flags) << ", " << in(op.in_slot[0]) << ", " << in(op.in_slot[1]) << ", " << m << "_c, pow_tabs);\n";
            break;
        case OP_NOISE:  // stateless: sample n of the voice's stream
            pro << "    const uint64_t " << m << "_key = noise_voice_key((uint64_t)__double_as_longlong(a.ops[" << k << "].delta), (uint64_t)__double_as_longlong(a.ops[" << k
                << "].sample_rate) + vc);\n";
            body << "        const float " << m << "_y = noise_sample(" << m << "_key, a.n0 + t0 + (uint32_t)i);\n";
            break;
        default: break;
        }
        slot[op.out_slot[0]] = m + "_y";
        if (op.kind == OP_VCA || op.kind == OP_MIX || op.kind == OP_MATH || op.kind == OP_NONLIN) {
            std::set<int> deps;
            bool pure = true;
            for (int j = 0; j < 4; j++) pure = pure && pure_deps(op.kind == OP_MIX || j < 2 ? op.in_slot[j] : -1, deps);
            if (pure) of.pure[op.out_slot[0]] = deps;
        }
    }

    // A broken feedback edge: the sink reads what the source wrote buffer_size samples ago.
    //   buffer_size 1        last tick's value: a register (the voice table keeps it between launches);
    //   buffer_size 2..16    a ring of LDS rows, loaded from / stored to the voice table's state rows like any module state;
    //   buffer_size >= 32    a ring in HBM ([B][V] f32): the 32 values a tile reads were all written before the tile began, so
    //                        the reads are issued together at the tile's start and the sample loop is fully unrolled (the
    //                        prefetch array is indexed by the sample's position in the tile);
    //   buffer_size 17..31   the same ring read sample by sample (a tile may read what it has just written; a lane's own
    //                        loads and stores to one address stay in program order).
    void gen_delay(int k, const DevOp& op)
    {
        const int B = P.hdr.buffer_size;
        const bool global = (op.flags & DELAY_RING_GLOBAL) != 0;
        const bool prefetch = global && B >= kMixRowsHost;
        const std::string r = uniq + "ring" + std::to_string(op.aux) + (global ? "g" : "");
        const std::string m = "m" + std::to_string(k);
        if (!ring_declared[op.aux * 2 + (global ? 1 : 0)]) {
            ring_declared[op.aux * 2 + (global ? 1 : 0)] = true;
            if (!global && B == 1) {
                ring_check_of[op.aux] = "__builtin_fabsf(" + r + ") <= @";
                pro << "    float " << r << " = rowf(" << op.aux << ");\n";
                epi << "        put(" << op.aux << ", __float_as_uint(" << r << "));\n";
            } else if (!global) {
                {
                    std::string c;
                    for (int j = 0; j < B; j++) c += std::string(j ? " && " : "") + "__builtin_fabsf(" + r + "[" + std::to_string(j) + " * 64 + lane]) <= @";
                    ring_check_of[op.aux] = "(" + c + ")";
                }
                lds_rings << "    __shared__ float " << r << "[" << B << " * 64];\n";
                pro << "    for (int j = 0; j < " << B << "; j++) " << r << "[j * 64 + lane] = rowf(" << op.aux << " + j);\n";
                epi << "        for (int j = 0; j < " << B << "; j++) put(" << op.aux << " + j, __float_as_uint(" << r << "[j * 64 + lane]));\n";
                uses_ring_pos = true;
            } else {
                pro << "    float* const " << r << " = a.rings + (size_t)" << op.aux << " * " << B << "u * V;\n";
                if (prefetch) {
                    needs_full_unroll = true;
                    pro << "    uint32_t " << r << "_p0 = (uint32_t)(a.n0 % " << B << "u);\n";
                    pro << "    auto " << r << "_at = [&](int i) { const uint32_t p = " << r << "_p0 + (uint32_t)i; return p < " << B << "u ? p : p - " << B << "u; };\n";
                    // the tile's 32 values, fetched a tile ahead when the ring is long enough for the next tile's to be older than this tile too
                    const bool ahead = B >= 2 * kMixRowsHost;
                    pro << "    float " << r << "_fed[kMixRows], " << r << "_nxt[kMixRows];\n";
                    pro << "#pragma unroll\n    for (int i = 0; i < kMixRows; i++) { " << r << "_fed[i] = " << r << "[(size_t)" << r << "_at(i) * V + vc]; " << r << "_nxt[i] = 0.0f; }\n";
                    if (ahead)
                        tile_begin << "        if (t0 + kMixRows < a.T) {\n#pragma unroll\n            for (int i = 0; i < kMixRows; i++) " << r << "_nxt[i] = " << r << "[(size_t)" << r
                                   << "_at(kMixRows + i) * V + vc];\n        }\n";
                    tile_end << "        " << r << "_p0 = " << r << "_at(n);\n";
                    if (ahead)
                        tile_end << "#pragma unroll\n        for (int i = 0; i < kMixRows; i++) " << r << "_fed[i] = " << r << "_nxt[i];\n";
                    else
                        tile_end << "        if (t0 + kMixRows < a.T) {\n#pragma unroll\n            for (int i = 0; i < kMixRows; i++) " << r << "_fed[i] = " << r << "[(size_t)" << r
                                 << "_at(i) * V + vc];\n        }\n";
                } else {
                    uses_ring_pos = true;
                }
            }
        }
        if (op.kind == OP_DELAY_RD && !global && ring_check_of.count(op.aux)) ring_check[k] = ring_check_of[op.aux];
        if (op.kind == OP_DELAY_RD) {
            if (!global && B == 1)
                body << "        const float " << m << "_y = " << r << ";\n";
            else if (!global)
                body << "        const float " << m << "_y = " << r << "[ring_pos * 64 + lane];\n";
            else if (prefetch)
                body << "        const float " << m << "_y = " << r << "_fed[i];\n";
            else
                body << "        const float " << m << "_y = " << r << "[(size_t)ring_pos * V + vc];\n";
            slot[op.out_slot[0]] = m + "_y";
        } else {
            if (!global && B == 1)
                body << "        " << r << " = " << in(op.in_slot[0]) << ";\n";
            else if (!global)
                body << "        " << r << "[ring_pos * 64 + lane] = " << in(op.in_slot[0]) << ";\n";
            else if (prefetch)
                body << "        if (active) " << r << "[(size_t)" << r << "_at(i) * V + voice] = " << in(op.in_slot[0]) << ";\n";
            else
                body << "        if (active) " << r << "[(size_t)ring_pos * V + voice] = " << in(op.in_slot[0]) << ";\n";
        }
    }

    // The tables behind 2^cv (sample player) and log2 (NonLinear, default mode), copied to LDS once per launch: a lane's own index is a
    // ds_read there and a gather for the vector-memory pipe through the global pointer (modules.hip.h: LdsTables; P4 29.9 -> see NOTES).
    void want_lds_tables()
    {
        if (lds_tables) return;
        lds_tables = true;
        lds_rings << "    __shared__ uint64_t " << uniq << "pow_tabs_lds[64];\n";
        pro << "    " << uniq << "pow_tabs_lds[lane] = lane < 32 ? ((const uint64_t*)kPowfLog2Tab)[lane] : kExp2fTab[lane - 32];\n";
        pro << "    LdsTables pow_tabs;  // (assigned, not brace-initialised: a constant initialiser may not cast into the LDS address space)\n";
        pro << "    pow_tabs.log2_tab = (LdsTab*)" << uniq << "pow_tabs_lds;\n    pow_tabs.exp2f_tab = pow_tabs.log2_tab + 32;\n";
        needs_sync = true;
    }

    // Sequencers evaluated per voice (a per-voice clock, or everything per voice): the 64 grid cells are wave-shared data in an LDS
    // array indexed by step; each lane gathers the cell of its own current_step.
    void gen_seq(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        const int sr = op.state_row;
        const bool grid = op.kind == OP_GRIDSEQ;
        const bool bank = (op.flags & SEQ_BANK) != 0;
        // SEQ_BANK (a sequence per voice: srack_voices_set_sequences): the length and where the lane's 64 cells start behind the own ones are
        // per-lane registers read from the voice table, and the cell is gathered from the lane's own cells in seqtab — one load per sample,
        // 64 lanes in up to 64 sequences.  (Tried: the lane's 64 cells copied once per launch into a step-major LDS tile [64 steps][64 lanes],
        // 16 KB per sequencer, conflict-free whatever step each lane is on.  At P3's 262 144 voices — four waves per SIMD — two tiles leave
        // room for three workgroups per CU: 167 ms per step against the gather's 63.7.  Where a tile fits the kernel's LDS share, 65 536
        // voices, it won 2.3 ms of 32.7 with a clock per voice and tied on a shared clock: not kept.  tools/seq_bank_bench.py, notes/r12.md.)
        if (!bank) {
            lds_rings << "    __shared__ uint32_t " << uniq << m << "_cells_lds[64];\n";
            lds_rings << "    uint32_t* const " << m << "_cells = " << uniq << m << "_cells_lds;\n";
            pro << "    " << m << "_cells[lane] = a.seqtab[a.ops[" << k << "].aux + lane];\n";
            needs_sync = true;
        } else {
            pro << "    const uint32_t* const " << m << "_cells = a.seqtab + a.ops[" << k << "].aux + row(" << op.par_row[SEQ_P_CELL_OFF] << ");  // this lane's own 64 cells\n";
        }
        pro << "    SeqRegs " << m << ";\n    " << m << ".current_step = row(" << sr + SEQ_S_CURRENT << "); " << m << ".step_last = row(" << sr + SEQ_S_STEP_LAST << ") != 0; " << m
            << ".sync_last = row(" << sr + SEQ_S_SYNC_LAST << ") != 0;\n";
        if (bank)
            pro << "    const uint32_t " << m << "_len = row(" << op.par_row[SEQ_P_LEN] << ");  // this lane's sequence\n";
        else
            pro << "    const uint32_t " << m << "_len = (uint32_t)a.ops[" << k << "].seq_len;\n";
        const std::string step = in(op.in_slot[0]), sync = in(op.in_slot[1]);
        body << "        const float " << m << "_step = " << step << ";\n";
        body << "        const uint32_t " << m << "_cs = seq_advance(" << m << ", " << m << "_step, " << sync << ", " << m << "_len);\n";
        body << "        const uint32_t " << m << "_cell = " << m << "_cells[" << m << "_cs];\n";
        if (grid) {
            pro << "    float " << m << "_last = rowf(" << sr + GRIDSEQ_S_LAST << ");\n";
            pro << "    const float " << m << "_inv = 1.0f / " << par(k, GRIDSEQ_P_SPO) << ";  // 1.0 / steps_per_octave as f32 (sequencer.rs:236)\n";
            body << "        float " << m << "_y0, " << m << "_y1, " << m << "_y2;\n";
            body << "        gridseq_outputs(" << m << "_cell, " << m << "_cs, " << m << "_step, " << m << "_inv, " << m << "_last, " << m << "_y0, " << m << "_y1, " << m << "_y2);\n";
            for (int p = 0; p < 3; p++)
                if (op.out_slot[p] >= 0) slot[op.out_slot[p]] = m + "_y" + std::to_string(p);
            epi << "        put(" << sr + GRIDSEQ_S_LAST << ", __float_as_uint(" << m << "_last));\n";
        } else {
            for (int p = 0; p < 9; p++) {
                if (op.out_slot[p] < 0) continue;
                if (p == 8)
                    body << "        const float " << m << "_y8 = " << m << "_cs == 0u ? 1.0f : 0.0f;\n";
                else
                    body << "        const float " << m << "_y" << p << " = patseq_gate(" << m << "_cell, " << p << ", " << m << "_step);\n";
                slot[op.out_slot[p]] = m + "_y" + std::to_string(p);
            }
        }
        epi << "        put(" << sr + SEQ_S_CURRENT << ", " << m << ".current_step); put(" << sr + SEQ_S_STEP_LAST << ", " << m << ".step_last ? 1u : 0u); put(" << sr + SEQ_S_SYNC_LAST
            << ", " << m << ".sync_last ? 1u : 0u);\n";
    }

    // SampleModule (sample.rs:192-240): the position state machine, then one gather from the shared wave per sample.
    // SMP_BANK (a wave per voice: srack_voices_set_waves): the wave's length, the rate ratio and where the wave starts behind the own wave
    // are per-lane registers read from the voice table; everything else is the same text.
    void gen_sample(int k, const DevOp& op)
    {
        const std::string m = "m" + std::to_string(k);
        const int sr = op.state_row;
        const bool bank = (op.flags & SMP_BANK) != 0;
        want_lds_tables();
        pro << "    SmpRegs " << m << ";\n    " << m << ".pos = rowf(" << sr + SMP_S_POS << "); " << m << ".playing = row(" << sr + SMP_S_PLAYING << ") != 0; " << m << ".gate_last = row("
            << sr + SMP_S_GATE_LAST << ") != 0;\n";
        pro << "    const float " << m << "_ratio = " << par(k, SMP_P_WAVE_SR) << " / " << par(k, SMP_P_SR) << ";\n";
        if (bank) {
            pro << "    const uint32_t " << m << "_n = row(" << op.par_row[SMP_P_WAVE_LEN] << "), " << m << "_base = row(" << op.par_row[SMP_P_WAVE_OFF] << ");  // this lane's wave\n";
            pro << "    const uint32_t " << m << "_region = (uint32_t)a.ops[" << k << "].seq_len;  // the own wave and the whole bank\n";
        } else {
            pro << "    const uint32_t " << m << "_n = (uint32_t)a.ops[" << k << "].seq_len;\n";
        }
        // A short wave (a one-shot of up to kSmpLdsWave frames: 8 KB, which keeps eight one-wave workgroups on a CU) is copied to LDS once per
        // launch: a lane's read of its own position is a ds_read — ~100 cycles, and nothing the frame stores of the samples before it can alias —
        // where the gather through the global pointer is a trip to L2 per sample that the recurrence around it (the position of sample t + 1 needs
        // 2^cv of sample t) cannot be scheduled away from at two waves per SIMD (P4, rocprofv3: SQ_WAIT_ANY 47 % of the wave cycles).  Which of the
        // two a kernel does is part of its source (the wave's length class), like everything else about the program's structure.
        // ... as long as it does not cost the render its occupancy: with the copy the workgroup must still fit its share of the CU's 160 KB at the
        // waves per SIMD this render has — 10 KB at four (262 144 voices: sixteen one-wave workgroups per CU in ONE round; the mix tile and the
        // power tables already take 9.2 KB of it: no copy), 20 KB at two (P4's 131 072: the 8 KB copy fits).  In power-of-two classes from 256
        // frames.  (tools/patch_survey.py, 262 144 voices, one box: even a 2 KB copy for the fuzzer's 1 ... 400-frame waves put seeds 1 and 8 into a
        // second round of workgroups — 164 / 168 against 124 / 138 ms.)
        // With a bank the region that is staged is the own wave and the whole bank (op.seq_len): lanes read it at base + index.  The share is
        // the KERNEL's: every player's copy counts against it (three players with an 8 KB wave each used to pass the check one by one).
        int kSmpLdsWave = 256;
        while (kSmpLdsWave < op.seq_len && kSmpLdsWave < 2048) kSmpLdsWave *= 2;
        int lds_other = 1024 + ((out_mode & 2) ? 8704 : 0);  // tables, cells; one mix tile
        for (const DevOp& q : P.ops)
            if (q.kind == OP_DELAY_RD && !(q.flags & DELAY_RING_GLOBAL)) lds_other += (int)P.hdr.buffer_size * 256;
        const int lds_share = 160 * 1024 / (4 * std::max(1, std::min(want_waves > 0 ? want_waves : 2, 4))) - lds_other;
        const bool staged = knobs.smp_lds && !is_ctl && op.seq_len > 0 && op.seq_len <= kSmpLdsWave && smp_lds_bytes + 4 * kSmpLdsWave <= lds_share;
        if (staged) smp_lds_bytes += 4 * kSmpLdsWave;
        std::string read;  // the expression of the sample at index m_i
        if (staged && bank) {
            lds_rings << "    __shared__ uint32_t " << uniq << m << "_bank_lds[" << kSmpLdsWave << "];\n";
            pro << "    for (uint32_t q = (uint32_t)lane; q < " << m << "_region && q < " << kSmpLdsWave << "u; q += 64u) " << uniq << m << "_bank_lds[q] = (a.seqtab + a.ops[" << k << "].aux)[q];\n";
            read = uniq + m + "_bank_lds[" + m + "_base + " + m + "_i]";
            needs_sync = true;
        } else if (staged) {
            lds_rings << "    __shared__ uint32_t " << uniq << m << "_wave_lds[" << kSmpLdsWave << "];\n";
            pro << "    for (uint32_t q = (uint32_t)lane; q < " << m << "_n && q < " << kSmpLdsWave << "u; q += 64u) " << uniq << m << "_wave_lds[q] = (a.seqtab + a.ops[" << k << "].aux)[q];\n";
            pro << "    const uint32_t* const " << m << "_wave = " << uniq << m << "_wave_lds;\n";
            read = m + "_wave[" + m + "_i]";
            needs_sync = true;
        } else if (bank && knobs.smp_window) {
            // 64 lanes in 64 different waves: 64 cache lines per sample, and no copy to LDS is possible.  Each lane walks ITS wave nearly
            // sequentially, so it keeps the aligned group of four dwords around its index and the next one, loaded ahead, in registers
            // (modules.hip.h, SmpWindow): same memory, same bits, a quarter of the loads — none of them waited for while the lane plays on.
            // Measured (tools/bank_bench.py, P4 at 131 072 voices, 1024 waves of 48 000 frames, one box, three alternating rounds): 20.36 /
            // 20.39 / 20.43 ms per step against the plain gather's 22.16 / 22.20 / 22.15 (notes/r11.md).
            pro << "    SmpWindow " << m << "_win = smp_window_init();\n";
            pro << "    const uint32_t " << m << "_first = (uint32_t)a.ops[" << k << "].aux + " << m << "_base;  // the lane's wave in seqtab (dwords)\n";
            read = "smp_window_read(" + m + "_win, a.seqtab, " + m + "_first + " + m + "_i)";
        } else if (bank) {
            pro << "    const uint32_t* const " << m << "_wave = a.seqtab + a.ops[" << k << "].aux;  // (bank in global memory, plain gather)\n";
            read = m + "_wave[" + m + "_base + " + m + "_i]";
        } else {
            pro << "    const uint32_t* const " << m << "_wave = a.seqtab + a.ops[" << k << "].aux;\n";
            read = m + "_wave[" + m + "_i]";
        }
        body << "        const uint32_t " << m << "_i = sample_advance(" << hex(op.flags) << ", " << m << ", " << m << "_ratio, " << m << "_n, " << in(op.in_slot[0]) << ", " << in(op.in_slot[1])
             << ", pow_tabs);\n";
        body << "        const float " << m << "_y = __uint_as_float(" << m << "_n ? " << read << " : 0u);  // empty wave: `*out = 0.0`\n";
        slot[op.out_slot[0]] = m + "_y";
        epi << "        put(" << sr + SMP_S_POS << ", __float_as_uint(" << m << ".pos)); put(" << sr + SMP_S_PLAYING << ", " << m << ".playing ? 1u : 0u); put(" << sr + SMP_S_GATE_LAST << ", "
            << m << ".gate_last ? 1u : 0u);\n";
    }

    void gen_out(int k, const DevOp& op)
    {
        const std::string e = "em" + std::to_string(k);
        const int s = op.in_slot[0];
        if (is_ctl) {
            // a control unit's plane is a track [T] (one voice): lane j keeps sample j of the tile, one coalesced store per tile
            pro << "    float " << e << "_keep = 0.0f;\n";
            pro << "    float* const " << e << "_trk = a.frames + (size_t)" << op.aux << " * a.plane_stride;\n";
            body << "        " << e << "_keep = lane == i ? " << in(s) << " : " << e << "_keep;\n";
            tile_end << "        if (lane < n) " << e << "_trk[t0 + (uint32_t)lane] = " << e << "_keep;\n";
            return;
        }
        const bool frames = (out_mode & 1) != 0, mix = (out_mode & 2) != 0;
        pro << "    Emit " << e << " = make_emit(a, " << op.aux << ", lane);\n";
        if (s >= kTrackSlot) {  // every voice plays the same thing
            const int tk = s - kTrackSlot;
            const std::string v = in(s);
            body << "        emit_track_put(" << e << ", " << v << ", V, " << (frames ? "true" : "false") << ");\n";
            tile_end << "        emit_track_flush(" << e << ", (const float*)trk" << tk << "_v + t0, t0, n, V, " << (frames ? "true" : "false") << ", " << (mix ? "true" : "false") << ");\n";
            return;
        }
        const int tile = tile_of_out.count(k) ? tile_of_out[k] : 0;  // (without a mix-down the tile is never touched)
        if (rows_per_plane > 0 && tile_of_out.count(k)) {
            const int R = rows_per_plane;
            body << "        emit_put_rows<KOUT>(" << e << ", mix_tile + " << tile * R << " * kMixPitch, " << in(s) << ", i & " << R - 1 << ", V);\n";
            tile_end << "        emit_rows_end<KOUT>(" << e << ", n, V);\n";
            shared_emits.push_back(e);
            if (tile == (int)tile_of_out.size() - 1) {  // the last plane of the sample: every R samples (and at a ragged tile's end) all the planes' rows leave together
                pro << "    float* const mix_mp_lane = ";
                for (size_t j = 0; j < shared_emits.size(); j++) pro << "(lane & 31) / " << R << " == " << j << " ? " << shared_emits[j] << ".mp : ";
                pro << "nullptr;\n";
                body << "        if ((KOUT & 2) && ((i & " << R - 1 << ") == " << R - 1 << " || i == n - 1)) emit_rows_flush<" << R << ">(" << shared_emits[0]
                     << ", mix_tile, mix_mp_lane, t0 + (uint32_t)(i & ~" << R - 1 << "), (i & " << R - 1 << ") + 1);\n";
            }
            return;
        }
        body << "        emit_put<KOUT>(" << e << ", mix_tile + " << tile << " * kMixTile, " << in(s) << ", i, V);\n";
        tile_end << "        emit_flush<KOUT>(" << e << ", mix_tile + " << tile << " * kMixTile, t0, n, V);\n";
    }

    bool gen_ops()
    {
        for (int k = 0; k < (int)P.ops.size(); k++) {
            const DevOp& op = P.ops[(size_t)k];
            body << "        // op " << k << ": kind " << op.kind << " (module " << op.module << ")\n";
            in_facts = of.snapshot();  // (WireFacts: the op reads its inputs' facts, its outputs' old ones end here)
            for (int s : op.out_slot)
                if (s >= 0) of.overwrite(s);
            switch (op.kind) {
            case OP_OSC: gen_osc(k, op); break;
            case OP_VCF: gen_vcf(k, op); break;
            case OP_ADSR: gen_adsr(k, op); break;
            case OP_VCA:
            case OP_MIX:
            case OP_MATH:
            case OP_NONLIN:
            case OP_NOISE: gen_simple(k, op); break;
            case OP_DELAY_RD:
            case OP_DELAY_WR: gen_delay(k, op); break;
            case OP_OUT: gen_out(k, op); break;
            case OP_GRIDSEQ:
            case OP_PATSEQ: gen_seq(k, op); break;
            case OP_SAMPLE: gen_sample(k, op); break;
            default: err = "op kind " + std::to_string(op.kind) + " is not covered by the kernel generator"; break;
            }
            if (!err.empty()) return false;
        }
        return true;
    }

    // the body of a function whose argument block is `a` (a KernelArgs): everything between its braces
    void emit_function_body(std::ostream& o)
    {
        emit_prologue(o);
        const std::string loops = versioned_on_fast_conds(tile_loop());
        if (fm_ops.empty() || is_ctl) {
            o << loops;
        } else {  // versioned oscillators (analyze): the wave's vote, once per launch, then the copy of the loop compiled for its classes
            emit_fm_vote(o);
            emit_fm_dispatch(o, loops);
        }
        o << "    if (active) {\n" << epi.str() << "    }\n";
    }

    // ---- part 1: the lane map, `row` / `rowf` / `put`, the rings, the tracks, then what the ops declared (pro) ----
    void emit_prologue(std::ostream& o)
    {
        const DevProgram& H = P.hdr;
        if (!is_ctl) {
            if (n_tiles > 0)  // one transpose tile per plane that is fed by a wire (+ those only an exact saw oscillator uses)
                o << "    __shared__ __attribute__((aligned(16))) float mix_tile[" << n_tiles << " * kMixTile];\n";
            else  // no mix-down, no tile-wise oscillator: never touched
                o << "    __shared__ __attribute__((aligned(16))) float mix_tile[4];\n";
            o << "    (void)mix_tile;\n";
        }
        o << "    const int lane = threadIdx.x;\n";
        o << "    const WaveMap wm = wave_map(a, lane);\n";
        o << "    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;\n";
        o << "    const bool active = wm.active;\n";
        o << "    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };\n";
        o << "    auto rowf = [&](int rr) { return __uint_as_float(a.table[(size_t)rr * V + vc]); };\n";
        if (is_ctl) {
            // (a tick session: the rows nobody rewrites — parameters — travel to the next copy with the state; the fence orders these
            // stores before the epilogue's stores to the same rows, which another lane issues)
            o << "    uint32_t* const tout = a.table_out ? a.table_out : a.table;\n";
            o << "    if (a.table_out) {\n        for (uint32_t r = (uint32_t)lane; r < (uint32_t)a.prog.n_rows; r += 64u) a.table_out[r] = a.table[r];\n"
                 "        __builtin_amdgcn_fence(__ATOMIC_RELEASE, \"workgroup\");\n    }\n";
            o << "    auto put = [&](int rr, uint32_t v) { tout[(size_t)rr * V + voice] = v; };\n";
        } else {
            o << "    auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };\n";
        }
        o << "    const float zero_in = zero_f32();\n";
        o << "    (void)voice; (void)active; (void)row; (void)rowf; (void)put; (void)zero_in;\n";
        o << lds_rings.str();
        if (uses_ring_pos) o << "    uint32_t ring_pos = (uint32_t)(a.n0 % " << H.buffer_size << "u);  // wave-uniform: scalar arithmetic\n";
        for (int tk : tracks_used) {
            // a control track is wave-uniform data written by an earlier launch: read through the scalar unit (constant address space)
            o << "    const float* const trk" << tk << "_v = a.tracks + (size_t)" << H.track_id[tk] << " * a.t_stride;\n";
            o << "    CFloat* const trk" << tk << " = (CFloat*)(uintptr_t)trk" << tk << "_v;\n";
        }
        o << pro.str();
        if (needs_sync) o << "    __syncthreads();\n";
        if (is_ctl)
            for (int tk : tracks_used) o << "    float trk" << tk << "_nx = trk" << tk << "_v[min((uint32_t)lane, a.T - 1u)];\n";
    }

    // how far the sample loop is unrolled: straight-line code lets the scheduler overlap independent recurrences of
    // neighbouring samples (the oscillator of t+1 beside the filter of t), but the body must stay inside the instruction cache
    int unroll_factor() const
    {
        int weight = 0;
        // (NonLinear: a table-driven power with ocml's powf behind a wave-uniform branch for the special cases — ~300 instructions a sample;
        // unrolled 32 times P4's loop was 11 000 instructions, 75 KB, more than the instruction cache two CUs share: 94 VALU instructions
        // took 677 SIMD cycles per wave-sample, and MORE with four waves per SIMD than with two)
        for (const DevOp& op : P.ops)
            weight += op.kind == OP_OSC ? ((op.flags & OSC_CONST_FAST) ? 2 : 8)
                    : op.kind == OP_VCF ? 4 : op.kind == OP_ADSR ? 3 : op.kind == OP_NONLIN ? 20 : (op.kind == OP_SAMPLE && (op.flags & SMP_HAS_CV)) ? 4 : 1;
        int unroll = needs_full_unroll ? 32 : is_ctl ? 4 : (weight <= 10 ? 32 : (weight <= 24 ? 8 : 4));
        if (knobs.unroll_cap >= 1 && !needs_full_unroll && !is_ctl) unroll = std::min(unroll, knobs.unroll_cap);
        return unroll;
    }

    // The input tracks at sample i and what the ops asked to be fetched ahead (sample_args): as the sample function's parameters, and as
    // its arguments called directly at sample `i` or from arrays loaded a group of samples ahead.
    struct SampleArgs {
        std::string params, direct, group_decl, group_load, group_args;
    };
    SampleArgs sample_arg_texts() const
    {
        SampleArgs s;
        if (!is_ctl)
            for (int tk : tracks_used) {
                const std::string t = std::to_string(tk);
                s.params += ", float tk" + t;
                s.direct += ", trk" + t + "[t0 + (uint32_t)i]";
                s.group_decl += "                float tg" + t + "[kGroup];\n";
                s.group_load += " tg" + t + "[u] = trk" + t + "[t0 + (uint32_t)(i0 + u)];";
                s.group_args += ", tg" + t + "[u]";
            }
        for (const auto& sa : sample_args) {
            auto at = [&](const std::string& idx) {  // the expression with `i` replaced
                std::string e = sa.second;
                const size_t p0 = e.find("(i)");
                if (p0 != std::string::npos) e.replace(p0, 3, "(" + idx + ")");
                return e;
            };
            s.params += ", float " + sa.first;
            s.direct += ", " + at("i");
            s.group_decl += "                float " + sa.first + "_g[kGroup];\n";
            s.group_load += " " + sa.first + "_g[u] = " + at("i0 + u") + ";";
            s.group_args += ", " + sa.first + "_g[u]";
        }
        return s;
    }

    // ---- part 2: the loop over tiles of kMixRows samples: the sample function (the ops' body), and one of four ways of driving it ----
    std::string tile_loop()
    {
        std::ostringstream o;
        const int unroll = unroll_factor();
        o << "    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {\n";
        o << "        const int n = (int)min((uint32_t)kMixRows, a.T - t0);\n";
        if (is_ctl)
            for (int tk : tracks_used) {
                o << "        const float trk" << tk << "_t = trk" << tk << "_nx;\n";
                o << "        trk" << tk << "_nx = trk" << tk << "_v[min(t0 + (uint32_t)kMixRows + (uint32_t)lane, a.T - 1u)];  // the next tile, in flight while this one runs\n";
            }
        o << tile_begin.str();
        const SampleArgs sa = sample_arg_texts();
        const bool quiet = !quiet_lane.empty() && !is_ctl && !across_lanes && !needs_full_unroll;
        o << group_decl.str();  // (also without quiet groups: the discarded arm of a non-generic lambda's `if constexpr` is still looked up)
        if (quiet)
            o << "        auto sample = [&](auto quiet_c, int i" << sa.params << ") {\n            constexpr bool kQuiet = decltype(quiet_c)::value != 0u;\n";
        else
            o << "        auto sample = [&](int i" << sa.params << ") {\n            constexpr bool kQuiet = false;\n            (void)kQuiet;\n";
        o << indent(body.str(), 4);
        if (uses_ring_pos) o << "            ring_pos = ring_pos + 1u == " << P.hdr.buffer_size << "u ? 0u : ring_pos + 1u;\n";
        o << "        };\n";
        if (quiet) {
            emit_quiet_groups(o, sa);
        } else if (across_lanes) {  // every statement of the body is a whole tile: lane j computes sample j
            o << "        sample(lane);\n";
        } else if (needs_full_unroll) {
            o << "#pragma unroll\n        for (int i = 0; i < kMixRows; i++)\n            if (i < n) sample(i" << sa.direct << ");\n";
        } else if (sa.params.empty()) {
            o << "        if (n == kMixRows) {\n#pragma unroll " << unroll << "\n            for (int i = 0; i < kMixRows; i++) sample(i);\n        } else {\n"
              << "            for (int i = 0; i < n; i++) sample(i);\n        }\n";
        } else {
            // Track values are fetched a group of samples at a time, ahead of the group's arithmetic (adjacent scalar loads merge into
            // s_load_dwordx4/x8): a load per sample, each behind the branches of the sample before it, would be waited for every time.
            const int group = std::min(unroll, 8);
            o << "        if (n == kMixRows) {\n            constexpr int kGroup = " << group << ";\n#pragma unroll " << unroll / group
              << "\n            for (int i0 = 0; i0 < kMixRows; i0 += kGroup) {\n" << sa.group_decl
              << "#pragma unroll\n                for (int u = 0; u < kGroup; u++) {" << sa.group_load << " }\n"
              << "#pragma unroll\n                for (int u = 0; u < kGroup; u++) sample(i0 + u" << sa.group_args << ");\n            }\n        } else {\n"
              << "            for (int i = 0; i < n; i++) sample(i" << sa.direct << ");\n        }\n";
        }
        o << tile_end.str();
        o << "    }\n";
        return o.str();
    }

    // groups of kQuietGroup samples: the quiet copy of the sample function where no lane can have an event within the group, the literal
    // per-sample copy, unrolled, for the whole group where one can
    void emit_quiet_groups(std::ostream& o, const SampleArgs& sa) const
    {
        o << "        if (n == kMixRows) {\n            constexpr int kGroup = kQuietGroup;\n#pragma unroll 1\n            for (int i0 = 0; i0 < kMixRows; i0 += kGroup) {\n"
          << sa.group_decl;
        if (!sa.group_load.empty()) o << "#pragma unroll\n                for (int u = 0; u < kGroup; u++) {" << sa.group_load << " }\n";
        // (track values of a group sit in arrays indexed from the group's first sample: sample i of a run is element i & 7)
        std::string sub_args = sa.group_args;
        for (size_t at = sub_args.find("[u]"); at != std::string::npos; at = sub_args.find("[u]", at)) sub_args.replace(at, 3, "[(i1 + u) & (kGroup - 1)]");
        // run samples [i1, i1 + kLen) through the event-free copy if no lane can have an event within them; says whether it did
        o << "                auto quiet_run = [&](auto len_c, int i1) -> bool {\n                    constexpr int kLen = (int)decltype(len_c)::value;\n"
          << "                    constexpr int kLi = kLen == 8 ? 0 : (kLen == 4 ? 1 : (kLen == 2 ? 2 : 3));\n                    (void)kLi;\n"
          << indent(group_begin.str(), 4) << "                    bool quiet_lane = true;\n";
        for (const auto& c : quiet_lane) o << "                    quiet_lane = quiet_lane && " << c << ";\n";
        o << "                    if (__builtin_amdgcn_ballot_w64(!quiet_lane) != 0) return false;\n#pragma unroll\n                    for (int u = 0; u < kLen; u++) sample(UC<1u>{}, i1 + u"
          << sub_args << ");\n" << group_end_quiet.str() << "                    return true;\n                };\n";
        o << "                if (!quiet_run(UC<8u>{}, i0)) {\n";
        o << "#pragma unroll " << knobs.nq_unroll << "\n                    for (int u = 0; u < kGroup; u++) sample(UC<0u>{}, i0 + u" << sa.group_args << ");\n";
        o << "                }\n            }\n        } else {\n            for (int i = 0; i < n; i++) sample(UC<0u>{}, i" << sa.direct << ");\n        }\n";
    }

    // ---- part 3: the loop in as many copies as there are launch-uniform conditions to version it on ----
    std::string versioned_on_fast_conds(const std::string& loop_text) const
    {
        if (fast_conds.empty() || is_ctl) return loop_text;
        std::ostringstream loops;
        loops << "    if (";
        for (size_t c = 0; c < fast_conds.size(); c++) loops << (c ? " && " : "") << fast_conds[c].first;
        loops << ") {  // the common case: these hold for the whole launch and are constants inside this copy of the loop\n";
        for (const auto& fc : fast_conds) loops << "    " << fc.second << "\n";
        loops << loop_text << "    } else {\n" << loop_text << "    }\n";
        return loops.str();
    }

    // ---- part 4: what the wave can prove about its versioned oscillators (analyze) for the whole launch, and the class of each ----
    void emit_fm_vote(std::ostream& out) const
    {
        const int nf = (int)fm_ops.size(), n_cls = fm_classes();
        std::set<int> oscs, rings;
        std::set<std::string> also;
        out << "    // what this wave can prove about its oscillators' pitch CVs for the whole launch (every lane votes; NaNs vote no)\n";
        for (int j = 0; j < nf; j++) {
            const int k = fm_ops[(size_t)j];
            const Fact& f = cv_fact[(size_t)k];
            out << "    const float fm_b" << j << " = " << f.bound << ";  // |cv| of op " << k << "\n";
            oscs.insert(f.oscs.begin(), f.oscs.end());
            oscs.insert(k);
            rings.insert(f.rings.begin(), f.rings.end());
            also.insert(f.also.begin(), f.also.end());
        }
        out << "    bool fm_lane = true;\n";
        for (const auto& c : also) out << "    fm_lane = fm_lane && " << c << ";\n";
        for (int j = 0; j < nf; j++) {  // the exponent val + cv stays clear of 2^x's overflow, 440 / sr is finite
            const std::string m = "m" + std::to_string(fm_ops[(size_t)j]);
            out << "    fm_lane = fm_lane && (double)fm_b" << j << " + __builtin_fabs(" << m << "_k.val) < 1000.0 && " << m << "_k.sr >= 1.0 && osc_below_rate(fm_b" << j << ", " << m
                << "_k.val, " << m << "_k.sr);\n";
        }
        for (int k : oscs) {  // phases in [0, 1) now; increments finite and >= 0 keep them there
            const auto pe = osc_pos.find(k);
            if (pe == osc_pos.end()) {
                out << "    fm_lane = false;  // (op " << k << ": an oscillator form without a phase to look at)\n";
                continue;
            }
            out << "    fm_lane = fm_lane && " << pe->second << " >= 0.0 && " << pe->second << " < 1.0;\n";
            const auto de = osc_delta.find(k);
            if (de != osc_delta.end() && !de->second.empty()) out << "    fm_lane = fm_lane && " << de->second << " >= 0.0 && " << de->second << " < 1.0e300;\n";
        }
        for (int rd : rings) {  // what a delayed edge hands over first is the host's (a rack file's saved buffer), not the source's
            const auto rc = ring_check.find(rd);
            if (rc == ring_check.end()) {
                out << "    fm_lane = false;\n";
                continue;
            }
            std::string c = rc->second;
            for (size_t at; (at = c.find('@')) != std::string::npos;) c.replace(at, 1, rd_fact[(size_t)rd].bound);
            out << "    fm_lane = fm_lane && " << c << ";\n";
        }
        out << "    const bool fm_ok = __builtin_amdgcn_ballot_w64(!fm_lane) == 0;\n";
        for (int j = 0; j < nf; j++) {
            // fm_gain_class: 2 = |cv| <= 1/2, 1 = |cv| <= 2, 0 = neither  ->  class 3 / 2 / 1 (with the classes this many oscillators share)
            const std::string g = "fm_g" + std::to_string(j);
            out << "    const int " << g << " = fm_gain_class(fm_b" << j << ");\n";
            out << "    const int fm_k" << j << " = " << (n_cls == 3 ? g + " + 1;\n" : n_cls == 2 ? g + " == 2 ? 3 : 1;\n" : "1;\n    (void)" + g + ";\n");
        }
    }

    // ... and the loops as a function of the classes, called with the combination the wave voted for (all literal when the vote failed)
    void emit_fm_dispatch(std::ostream& out, const std::string& loops) const
    {
        const int nf = (int)fm_ops.size(), n_cls = fm_classes();
        out << "    auto fm_run = [&](";
        for (int j = 0; j < nf; j++) out << (j ? ", " : "") << "auto fm_c" << j;
        out << ") {\n";
        for (int j = 0; j < nf; j++) out << "    constexpr uint32_t kFm" << j << " = fm_class_flags(decltype(fm_c" << j << ")::value);\n";
        out << loops << "    };\n";
        static const int kAllowed[4][3] = {{}, {1}, {1, 3}, {1, 2, 3}};
        const int* allowed = kAllowed[n_cls];
        out << "    if (!fm_ok) {\n        fm_run(";
        for (int j = 0; j < nf; j++) out << (j ? ", " : "") << "UC<0u>{}";
        out << ");\n    }";
        std::vector<int> pick((size_t)nf, 0);
        for (;;) {
            out << " else if (";
            for (int j = 0; j < nf; j++) out << (j ? " && " : "") << "fm_k" << j << " == " << allowed[pick[(size_t)j]];
            out << ") {\n        fm_run(";
            for (int j = 0; j < nf; j++) out << (j ? ", " : "") << "UC<" << allowed[pick[(size_t)j]] << "u>{}";
            out << ");\n    }";
            int j = 0;
            while (j < nf && ++pick[(size_t)j] == n_cls) pick[(size_t)j++] = 0;
            if (j == nf) break;
        }
        out << "\n";
    }
};

void emit_preamble(std::ostream& o, const GenKnobs& knobs, int out_mode, bool libm_tab_lds)
{
    // (nothing here may depend on more than the program's structure: the text is the cache key.  The flattener's description of the
    // program — it mentions the interpreter's tile length, which moves with the voice count — is added for human readers only,
    // by srack_render_kernel_source.)
    o << "// generated by s-rack_amd/csrc/jit.cpp\n";
    o << "#define SRK_OPAQUE_ZERO 1\n";
    if (libm_tab_lds) o << "#define SRK_LIBM_TAB_LDS 1  // pow's table in LDS: an exact oscillator's pitch moves (modules.hip.h)\n";
    if (knobs.quiet_group) o << "#define SRK_QUIET_GROUP " << knobs.quiet_group << "\n";
    o << "#include \"wave.hip.h\"\n";
    o << "using namespace srack;\nusing namespace srack::dev;\n";
    o << "typedef const __attribute__((address_space(4))) float CFloat;\n";
    o << "#define KOUT " << out_mode << "\n";
}
}  // namespace

bool jit_supported(const FlatProgram& P, std::string* why)
{
    auto no = [&](const std::string& w) {
        if (why) *why = w;
        return false;
    };
    if (P.ops.empty()) return no("empty program");
    int n_planes_wire = 0;
    for (const DevOp& op : P.ops) {
        switch (op.kind) {
        case OP_OSC: case OP_VCF: case OP_ADSR: case OP_VCA: case OP_MIX: case OP_MATH: case OP_NONLIN: case OP_NOISE:
        case OP_GRIDSEQ: case OP_PATSEQ: case OP_SAMPLE: case OP_DELAY_RD: case OP_DELAY_WR: break;
        case OP_OUT: n_planes_wire += op.in_slot[0] < kTrackSlot; break;
        default: return no("op kind " + std::to_string(op.kind) + (op.kind == OP_FREEVERB ? " (FreeverbModule)" : ""));
        }
    }
    if (n_planes_wire > 4) return no("more than four distinct output planes");  // one LDS mix tile each
    if ((int)P.ops.size() > 48) return no("more than 48 ops: the state would not stay in registers");
    return true;
}

bool jit_ctl_supported(const FlatPair& pair, std::string* why)
{
    if (pair.n_tracks <= 0 || pair.ctl.empty()) {
        if (why) *why = "no control program";
        return false;
    }
    for (const FlatProgram& c : pair.ctl)
        if (!jit_supported(c, why)) return false;
    return true;
}

// One kernel: the voice program, and — with_ctl — the control program's units as blocks [0, block0) of the same launch.
int jit_source(const FlatPair& pair, int out_mode, bool with_ctl, std::string& src, int waves_budget, int want_waves)
{
    const FlatProgram& P = pair.voice;
    std::string why;
    if (!jit_supported(P, &why) || (with_ctl && !jit_ctl_supported(pair, &why))) {
        set_error("specialise: " + why);
        return SRACK_ERR_UNSUPPORTED;
    }
    const GenKnobs knobs = read_knobs();
    std::ostringstream o;
    const int n_units = with_ctl ? (int)pair.ctl.size() : 0;
    // pow's table in LDS where an exact oscillator's pitch moves (the lookup is inside its recurrence)
    auto moving_exact = [](const FlatProgram& Q) {
        for (const DevOp& op : Q.ops)
            if (op.kind == OP_OSC && (op.flags & (OSC_EXACT | OSC_HAS_CV)) == (OSC_EXACT | OSC_HAS_CV)) return true;
        return false;
    };
    bool libm_tab_lds = moving_exact(P);
    for (int u = 0; u < n_units; u++) libm_tab_lds = libm_tab_lds || moving_exact(pair.ctl[(size_t)u]);
    emit_preamble(o, knobs, out_mode, libm_tab_lds);
    for (int u = 0; u < n_units; u++) {
        Gen g(pair.ctl[(size_t)u], knobs, 1, true, "u" + std::to_string(u) + "_");
        if (!g.gen_ops()) {
            set_error("specialise (control unit " + std::to_string(u) + "): " + g.err);
            return SRACK_ERR_UNSUPPORTED;
        }
        o << "// control unit " << u << "\n";
        o << "static __device__ __forceinline__ void srk_ctl" << u << "(const KernelArgs& a)\n{\n";
        o << "    if (a.T == 0) return;  // an idle slot of the pipeline\n";
        g.emit_function_body(o);
        o << "}\n\n";
    }
    Gen g(P, knobs, out_mode);
    g.want_waves = want_waves;
    if (!g.gen_ops()) {
        set_error("specialise: " + g.err);
        return SRACK_ERR_UNSUPPORTED;
    }
    {
        // a register budget for so many waves per SIMD (jit_get decides; SRACK_JIT_WAVES overrides) — the compiler's default for a
        // 64-thread workgroup is "all 512 registers"
        const int waves = knobs.waves_set ? knobs.waves : waves_budget;
        o << "extern \"C\" __global__ __launch_bounds__(64) ";
        if (waves >= 1 && waves <= 8) o << "__attribute__((amdgpu_waves_per_eu(" << waves << ", 8))) ";
        o << "void srk_voice(KernelArgs a)\n{\n";
        if (libm_tab_lds) o << "    libm_tab_fill((int)threadIdx.x);\n";
    }
    if (n_units > 0) {
        // Blocks [0, block0) are not voice waves: block b evaluates control unit b for a LATER chunk while the voice blocks
        // consume tracks an earlier launch finished (render.hip).  Same stream, no events, no second hardware queue.  A unit is a
        // latency chain sharing its SIMD with throughput-bound voice waves: without priority it can outlast them.
        o << "    if (blockIdx.x < a.block0) {\n        __builtin_amdgcn_s_setprio(3);\n        const KernelArgs c = a.ctl_slots[blockIdx.x];\n";
        o << "        switch (blockIdx.x) {\n";
        for (int u = 0; u < n_units; u++) o << "        case " << u << ": srk_ctl" << u << "(c); break;\n";
        o << "        default: break;\n        }\n        return;\n    }\n";
    }
    g.emit_function_body(o);
    o << "}\n";
    src = o.str();
    return SRACK_OK;
}
}  // namespace srack
