// capi.cpp — the extern "C" boundary declared in include/srack_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "freeverb_params.hpp"
#include "jit.hpp"
#include "runtime.hpp"

using namespace srack;

namespace srack {  // srk.cpp
int load_srk(const uint8_t* bytes, size_t n_bytes, Graph& g);
std::vector<uint8_t> save_srk(const Graph& g);
}

struct srack_patch {
    PatchHandle h;
};

#define CHECK_HANDLE(p)                       \
    do {                                      \
        if (!(p)) {                           \
            set_error("null patch handle");   \
            return SRACK_ERR_INVALID;         \
        }                                     \
    } while (0)

// No C++ exception may cross the C boundary (a Rust or ctypes host cannot unwind it): allocation failures become
// SRACK_ERR_NOMEM, anything else SRACK_ERR_INVALID with the text in srack_last_error().
template <class F>
static int guarded(F&& f) noexcept
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        try { set_error("out of memory"); } catch (...) {}
        return SRACK_ERR_NOMEM;
    } catch (const std::exception& e) {
        try { set_error(std::string("internal error: ") + e.what()); } catch (...) {}
        return SRACK_ERR_INVALID;
    } catch (...) {
        try { set_error("internal error"); } catch (...) {}
        return SRACK_ERR_INVALID;
    }
}

// `(int)x` of a NaN or of a value outside int's range is undefined: flags and enum-like fields are clamped first
static double as_flag(double x)
{
    if (!(x == x)) return 0.0;
    if (x > 2147483647.0) return 2147483647.0;
    if (x < -2147483648.0) return -2147483648.0;
    return (double)(int)x;
}

template <typename T>
static int set_voice_field_impl(srack_patch* p, int module, int field, const T* values)
{
    CHECK_HANDLE(p);
    PatchHandle& h = p->h;
    if (h.n_voices == 0) {
        set_error("voices_set_field: call srack_voices_configure first");
        return SRACK_ERR_STATE;
    }
    int nf = h.graph.num_fields(module);
    if (nf < 0 || field < 0 || field >= nf || !values) {
        set_error("voices_set_field: no such module/field");
        return SRACK_ERR_INVALID;
    }
    VoiceOverride o;
    o.module = module;
    o.field = field;
    o.values.resize(h.n_voices);
    const int type = h.graph.modules[(size_t)module].type;
    const bool f64 = Graph::field_is_f64(type, field), flag = Graph::field_is_flag(type, field);
    for (uint32_t v = 0; v < h.n_voices; v++) {
        double x = (double)values[v];
        o.values[v] = f64 ? x : (flag ? as_flag(x) : (double)(float)x);
    }
    for (auto it = h.overrides.begin(); it != h.overrides.end();)
        it = (it->module == module && it->field == field) ? h.overrides.erase(it) : it + 1;
    h.overrides.push_back(std::move(o));
    h.voices_revision++;
    if (Graph::field_is_state(type, field)) h.state_writes.insert({module, field});  // keep_state: the host's value wins over the carried one
    return SRACK_OK;
}

template <typename T>
static int set_voice_field(srack_patch* p, int module, int field, const T* values)
{
    return guarded([&]() -> int { return set_voice_field_impl(p, module, field, values); });
}

extern "C" {

int srack_abi_version(void) { return SRACK_ABI_VERSION; }
const char* srack_last_error(void) { return last_error(); }

int srack_patch_create(uint32_t sample_rate, uint32_t buffer_size, uint32_t channels, srack_patch** out)
{
    return guarded([&]() -> int {
        if (!out) {
            set_error("srack_patch_create: out is null");
            return SRACK_ERR_INVALID;
        }
        *out = nullptr;
        if (sample_rate == 0 || sample_rate > 65535u) {  // AudioConfig.sample_rate is a u16 (synth.rs:22)
            set_error("srack_patch_create: sample_rate must fit the reference's u16 (1..65535)");
            return SRACK_ERR_INVALID;
        }
        if (buffer_size == 0) {
            set_error("srack_patch_create: buffer_size must be >= 1");
            return SRACK_ERR_INVALID;
        }
        if (channels == 0 || channels > 8) {
            set_error("srack_patch_create: channels must be 1..8");
            return SRACK_ERR_INVALID;
        }
        auto* p = new (std::nothrow) srack_patch();
        if (!p) return SRACK_ERR_NOMEM;
        p->h.graph.cfg = AudioConfig{sample_rate, buffer_size, channels};
        *out = p;
        return SRACK_OK;
    });
}

int srack_patch_destroy(srack_patch* p)
{
    return guarded([&]() -> int {
        delete p;
        return SRACK_OK;
    });
}

int srack_patch_add_module(srack_patch* p, int module_type)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.add_module(module_type);
    });
}

int srack_patch_num_modules(const srack_patch* p)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return (int)p->h.graph.modules.size();
    });
}

static const Module* get_module(const srack_patch* p, int module)
{
    if (!p || module < 0 || module >= (int)p->h.graph.modules.size()) {
        set_error("no such module");
        return nullptr;
    }
    return &p->h.graph.modules[(size_t)module];
}

int srack_patch_module_type(const srack_patch* p, int module)
{
    return guarded([&]() -> int {
        const Module* m = get_module(p, module);
        return m ? m->type : SRACK_ERR_INVALID;
    });
}

int srack_module_num_inputs(const srack_patch* p, int module)
{
    return guarded([&]() -> int {
        const Module* m = get_module(p, module);
        return m ? m->n_in : SRACK_ERR_INVALID;
    });
}

int srack_module_num_outputs(const srack_patch* p, int module)
{
    return guarded([&]() -> int {
        const Module* m = get_module(p, module);
        return m ? m->n_out : SRACK_ERR_INVALID;
    });
}

int srack_patch_set_field(srack_patch* p, int module, int field, double value)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const int rc = p->h.graph.set_field(module, field, value);
        if (rc == SRACK_OK && Graph::field_is_state(p->h.graph.modules[(size_t)module].type, field)) {
            // keep_state: the host's value wins over the running one — also over the per-voice values an earlier carry left behind
            PatchHandle& h = p->h;
            h.state_writes.insert({module, field});
            if (h.keep_state)
                for (auto it = h.overrides.begin(); it != h.overrides.end();) it = (it->module == module && it->field == field) ? h.overrides.erase(it) : it + 1;
        }
        return rc;
    });
}

int srack_patch_get_field(const srack_patch* p, int module, int field, double* value)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.get_field(module, field, value);
    });
}

int srack_patch_set_step(srack_patch* p, int module, int channel, int step, int state, int value)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.set_step(module, channel, step, state, value);
    });
}

int srack_patch_get_step(const srack_patch* p, int module, int channel, int step, int* state, int* value)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.get_step(module, channel, step, state, value);
    });
}

int srack_patch_set_wave(srack_patch* p, int module, const float* samples, uint32_t n_samples, float sample_rate)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.set_wave(module, samples, n_samples, sample_rate);
    });
}

int srack_patch_get_wave(const srack_patch* p, int module, float* samples, uint32_t cap, float* sample_rate)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_module(p, module);
        if (!m || m->type != SRACK_MOD_SAMPLE) {
            set_error("get_wave: not a SampleModule");
            return SRACK_ERR_INVALID;
        }
        if (samples)
            for (size_t i = 0; i < m->wave.size() && i < (size_t)cap; i++) samples[i] = m->wave[i];
        if (sample_rate) *sample_rate = (float)m->fields[SRACK_SAMPLE_WAVE_SAMPLE_RATE];
        return (int)m->wave.size();
    });
}

int srack_patch_set_wave_bank(srack_patch* p, int module, const float* samples, const int* lengths, const float* sample_rates, uint32_t n_waves)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const int rc = p->h.graph.set_wave_bank(module, samples, lengths, sample_rates, n_waves);
        if (rc == SRACK_OK) p->h.voices_revision++;  // (the assignment, if there was one, is gone)
        return rc;
    });
}

static const Module* get_player(const srack_patch* p, int module, const char* who)
{
    const Module* m = get_module(p, module);
    if (!m || m->type != SRACK_MOD_SAMPLE) {
        set_error(std::string(who) + ": not a SampleModule");
        return nullptr;
    }
    return m;
}

int srack_patch_get_wave_bank(const srack_patch* p, int module, int* lengths, float* sample_rates, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_player(p, module, "get_wave_bank");
        if (!m) return SRACK_ERR_INVALID;
        for (size_t k = 0; k < m->bank_len.size() && k < (size_t)cap; k++) {
            if (lengths) lengths[k] = m->bank_len[k];
            if (sample_rates) sample_rates[k] = m->bank_sr[k];
        }
        return (int)m->bank_len.size();
    });
}

int srack_patch_get_wave_bank_samples(const srack_patch* p, int module, int wave, float* samples, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_player(p, module, "get_wave_bank_samples");
        if (!m) return SRACK_ERR_INVALID;
        if (wave < 0 || wave >= (int)m->bank_len.size()) {
            set_error("get_wave_bank_samples: no such wave");
            return SRACK_ERR_INVALID;
        }
        size_t first = 0;
        for (int k = 0; k < wave; k++) first += (size_t)m->bank_len[(size_t)k];
        const size_t n = (size_t)m->bank_len[(size_t)wave];
        if (samples)
            for (size_t i = 0; i < n && i < (size_t)cap; i++) samples[i] = (*m->bank)[first + i];
        return (int)n;
    });
}

int srack_voices_set_waves(srack_patch* p, int module, const int* wave)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        PatchHandle& h = p->h;
        if (!get_player(p, module, "voices_set_waves")) return SRACK_ERR_INVALID;
        if (h.n_voices == 0) {
            set_error("voices_set_waves: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        const int rc = h.graph.set_voice_waves(module, wave, h.n_voices);
        if (rc == SRACK_OK) h.voices_revision++;
        return rc;
    });
}

int srack_voices_get_waves(const srack_patch* p, int module, int* wave, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_player(p, module, "voices_get_waves");
        if (!m) return SRACK_ERR_INVALID;
        if (wave)
            for (size_t v = 0; v < m->voice_wave.size() && v < (size_t)cap; v++) wave[v] = m->voice_wave[v];
        return (int)m->voice_wave.size();
    });
}

static const Module* get_sequencer(const srack_patch* p, int module, const char* who)
{
    const Module* m = get_module(p, module);
    if (!m || (m->type != SRACK_MOD_GRID_SEQUENCER && m->type != SRACK_MOD_PATTERN_SEQUENCER)) {
        set_error(std::string(who) + ": not a sequencer");
        return nullptr;
    }
    return m;
}

int srack_patch_set_sequence_bank(srack_patch* p, int module, const void* states, const void* values, const int* lengths, uint32_t n_sequences)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const int rc = p->h.graph.set_sequence_bank(module, (const uint8_t*)states, (const uint16_t*)values, lengths, n_sequences);
        if (rc == SRACK_OK) p->h.voices_revision++;  // (the assignment, if there was one, is gone)
        return rc;
    });
}

int srack_patch_get_sequence_bank(const srack_patch* p, int module, void* states_out, void* values_out, int* lengths, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        uint8_t* const states = (uint8_t*)states_out;
        uint16_t* const values = (uint16_t*)values_out;
        const Module* m = get_sequencer(p, module, "get_sequence_bank");
        if (!m) return SRACK_ERR_INVALID;
        const bool grid = m->type == SRACK_MOD_GRID_SEQUENCER;
        const size_t C = grid ? 1 : 8;
        for (size_t k = 0; k < m->seq_bank_len.size() && k < (size_t)cap; k++) {
            if (lengths) lengths[k] = m->seq_bank_len[k];
            for (size_t step = 0; step < 64; step++) {
                const uint32_t cell = (*m->seq_bank)[k * 64 + step];
                if (grid) {
                    if (states) states[k * 64 + step] = (uint8_t)(!(cell & 0x80000000u) ? SRACK_STEP_NONE : ((cell & 0x40000000u) ? SRACK_STEP_HOLD : SRACK_STEP_ON));
                } else if (states) {
                    for (size_t c = 0; c < C; c++) {
                        const uint32_t b = (cell >> (2 * c)) & 3u;
                        states[(k * C + c) * 64 + step] = (uint8_t)(!(b & 1u) ? SRACK_STEP_NONE : ((b & 2u) ? SRACK_STEP_HOLD : SRACK_STEP_ON));
                    }
                }
                if (values) values[k * 64 + step] = grid ? (uint16_t)(cell & 0xffffu) : (uint16_t)0;
            }
        }
        return (int)m->seq_bank_len.size();
    });
}

int srack_voices_set_sequences(srack_patch* p, int module, const int* seq)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        PatchHandle& h = p->h;
        if (!get_sequencer(p, module, "voices_set_sequences")) return SRACK_ERR_INVALID;
        if (h.n_voices == 0) {
            set_error("voices_set_sequences: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        const int rc = h.graph.set_voice_sequences(module, seq, h.n_voices);
        if (rc == SRACK_OK) h.voices_revision++;
        return rc;
    });
}

int srack_voices_get_sequences(const srack_patch* p, int module, int* seq, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_sequencer(p, module, "voices_get_sequences");
        if (!m) return SRACK_ERR_INVALID;
        if (seq)
            for (size_t v = 0; v < m->voice_seq.size() && v < (size_t)cap; v++) seq[v] = m->voice_seq[v];
        return (int)m->voice_seq.size();
    });
}

int srack_patch_load_srk(const void* bytes, size_t n_bytes, uint32_t sample_rate, uint32_t buffer_size, uint32_t channels, srack_patch** out)
{
    return guarded([&]() -> int {
        if (!bytes && n_bytes) {
            set_error("srack_patch_load_srk: bytes is null");
            return SRACK_ERR_INVALID;
        }
        int rc = srack_patch_create(sample_rate, buffer_size, channels, out);
        if (rc != SRACK_OK) return rc;
        rc = load_srk((const uint8_t*)bytes, n_bytes, (*out)->h.graph);
        if (rc != SRACK_OK) {
            delete *out;
            *out = nullptr;
        }
        return rc;
    });
}

int srack_patch_save_srk(const srack_patch* p, void* buf, size_t cap, size_t* n_bytes)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        // The app saves the running rack: every module struct as it is at that moment.  With srack_patch_keep_state (voices running on
        // across edits) the file therefore carries the CURRENT state — of voice 0, a rack file being one instance — not the stored one.
        // (Port buffers are written as stored: only the sink of a broken feedback edge ever reads them.)
        PatchHandle& h = const_cast<srack_patch*>(p)->h;
        std::vector<uint8_t> bytes;
        if (h.keep_state && h.samples_rendered > 0) {
            // the running state: on the device while the program that rendered is still there (also after an edit the next render
            // has not picked up yet); otherwise where the last re-flatten committed it (fields, per-voice overrides: voice 0).
            // A state field the host wrote since keeps the host's value.
            Graph snap = h.graph;
            std::vector<double> values;
            for (int m = 0; m < (int)snap.modules.size(); m++) {
                Module& mod = snap.modules[(size_t)m];
                bool ran = false;
                for (int f = 0; f < (int)mod.fields.size(); f++) {
                    if (!Graph::field_is_state(mod.type, f) || h.state_writes.count({m, f})) continue;
                    if (h.prog_valid && h.dev && read_device_state(h, m, f, values)) {
                        mod.fields[(size_t)f] = values[0];
                        ran = true;
                    } else {
                        for (const auto& o : h.overrides)
                            if (o.module == m && o.field == f && !o.values.empty()) mod.fields[(size_t)f] = o.values[0];
                    }
                }
                if (ran && mod.type == SRACK_MOD_SAMPLE && mod.wave_revision <= h.prog_graph_revision) mod.fields[SRACK_SAMPLE_WAVE_NEW] = 0.0;  // consumed by the first tick (sample.rs:199-203)
            }
            bytes = save_srk(snap);
        } else {
            bytes = save_srk(h.graph);
        }
        if (n_bytes) *n_bytes = bytes.size();
        if (buf && cap < bytes.size()) {  // never hand back a truncated file that still parses as MessagePack up to the cut
            set_error("save_srk: buffer too small (" + std::to_string(cap) + " bytes, the file needs " + std::to_string(bytes.size()) + "); call with buf = NULL for the size");
            return SRACK_ERR_INVALID;
        }
        if (buf) std::memcpy(buf, bytes.data(), bytes.size());
        return SRACK_OK;
    });
}

int srack_patch_module_id(const srack_patch* p, int module, char* buf, size_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_module(p, module);
        if (!m) return SRACK_ERR_INVALID;
        if (buf && cap) std::snprintf(buf, cap, "%s", m->id.c_str());
        return (int)m->id.size();
    });
}

int srack_patch_set_module_position(srack_patch* p, int module, float x, float y)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (!get_module(p, module)) return SRACK_ERR_INVALID;
        Module& m = p->h.graph.modules[(size_t)module];
        m.has_pos = true;
        m.pos_x = x;
        m.pos_y = y;
        return SRACK_OK;
    });
}

int srack_patch_get_module_position(const srack_patch* p, int module, float* x, float* y)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Module* m = get_module(p, module);
        if (!m) return SRACK_ERR_INVALID;
        if (x) *x = m->pos_x;
        if (y) *y = m->pos_y;
        return m->has_pos ? 1 : 0;
    });
}

int srack_patch_set_output_buffer(srack_patch* p, int module, int port, const float* samples, uint32_t n)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.set_output_buffer(module, port, samples, n);
    });
}

int srack_patch_get_output_buffer(const srack_patch* p, int module, int port, float* dst, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const Graph& g = p->h.graph;
        if (module < 0 || module >= (int)g.modules.size()) {
            set_error("get_output_buffer: no such module");
            return SRACK_ERR_INVALID;
        }
        const Module& m = g.modules[(size_t)module];
        if (port < 0 || port >= m.n_out) {
            set_error("get_output_buffer: no such port");  // Err(()) of get_output
            return SRACK_ERR_PORT;
        }
        if ((size_t)port >= m.out_init.size()) return 0;
        const std::vector<float>& b = m.out_init[(size_t)port];
        if (dst)
            for (size_t i = 0; i < b.size() && i < (size_t)cap; i++) dst[i] = b[i];
        return (int)b.size();
    });
}

int srack_patch_keep_state(srack_patch* p, int keep)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (p->h.keep_state != (keep != 0)) p->h.graph.revision++;  // (the flattened program differs: with keep, every planned module is evaluated)
        p->h.keep_state = keep != 0;
        return SRACK_OK;
    });
}

int srack_patch_set_noise_seed(srack_patch* p, uint64_t seed, uint64_t first_voice)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        p->h.graph.cfg.noise_seed = seed;
        p->h.graph.cfg.noise_first_voice = first_voice;
        p->h.graph.revision++;  // the keys are part of the flattened program
        return SRACK_OK;
    });
}

int srack_patch_connect(srack_patch* p, int src_module, int src_port, int sink_module, int sink_port)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.connect(src_module, src_port, sink_module, sink_port);
    });
}

int srack_patch_disconnect(srack_patch* p, int sink_module, int sink_port)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return p->h.graph.disconnect(sink_module, sink_port);
    });
}

int srack_patch_get_input(const srack_patch* p, int sink_module, int sink_port, int* src_module, int* src_port)
{
    return guarded([&]() -> int {
        const Module* m = get_module(p, sink_module);
        if (!m) return SRACK_ERR_INVALID;
        if (sink_port < 0 || sink_port >= m->n_in) {
            set_error("get_input: port index out of range");
            return SRACK_ERR_PORT;
        }
        if (src_module) *src_module = m->in[(size_t)sink_port].src;
        if (src_port) *src_port = m->in[(size_t)sink_port].port;
        return SRACK_OK;
    });
}

int srack_patch_plan(srack_patch* p, int* order, int cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        Graph& g = p->h.graph;
        int n = g.make_plan();
        if (g.plan.output < 0) {
            set_error("plan: no OutputModule in the module list (plan is empty)");
            return SRACK_ERR_NO_OUTPUT;
        }
        for (int i = 0; i < n && i < cap && order; i++) order[i] = g.plan.order[(size_t)i];
        return n;
    });
}

int srack_patch_plan_list(srack_patch* p, int output, const int* all_modules, int n_all, int* order, int cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        Graph& g = p->h.graph;
        const int n_mod = (int)g.modules.size();
        if (output < 0 || output >= n_mod || !all_modules || n_all < 0) {
            set_error("plan_list: bad output / list");
            return SRACK_ERR_INVALID;
        }
        std::vector<int> all(all_modules, all_modules + n_all);
        for (int m : all)
            if (m < 0 || m >= n_mod) {
                set_error("plan_list: module index out of range");
                return SRACK_ERR_INVALID;
            }
        int n = g.make_plan(output, all);
        for (int i = 0; i < n && i < cap && order; i++) order[i] = g.plan.order[(size_t)i];
        g.plan.valid = false;  // a shuffled list is a test device; renders always plan in list order
        return n;
    });
}

int srack_patch_removed_edges(srack_patch* p, int* pairs, int cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const auto& r = p->h.graph.plan.removed;
        for (size_t i = 0; i < r.size() && (int)i < cap && pairs; i++) {
            pairs[2 * i] = r[i].first;
            pairs[2 * i + 1] = r[i].second;
        }
        return (int)r.size();
    });
}

int srack_patch_delayed_edges(srack_patch* p, int* quads, int cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        Graph& g = p->h.graph;
        if (!g.plan.valid) g.make_plan();
        auto edges = g.delayed_edges();
        for (size_t i = 0; i < edges.size() && (int)i < cap && quads; i++) {
            quads[4 * i + 0] = edges[i].src;
            quads[4 * i + 1] = edges[i].src_port;
            quads[4 * i + 2] = edges[i].sink;
            quads[4 * i + 3] = edges[i].sink_port;
        }
        return (int)edges.size();
    });
}

int srack_voices_configure(srack_patch* p, uint32_t n_voices)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (n_voices == 0 || n_voices > (1u << 24)) {  // a tile of 32 frame rows (32 * V * 4 bytes) must fit a 31-bit buffer offset
            set_error("voices_configure: n_voices must be 1 .. 16777216");
            return SRACK_ERR_INVALID;
        }
        p->h.n_voices = n_voices;
        p->h.overrides.clear();
        p->h.graph.drop_voice_waves();  // (no revision of the graph: voices_revision below re-flattens)
        p->h.voices_revision++;
        p->h.voices_fresh = true;
        p->h.n_buses = 0;  // the mix table belonged to the voices that were
        p->h.bus.clear();
        p->h.bus_gain.clear();
        p->h.bus_plan = BusPlan();
        p->h.bus_slots = 0;
        p->h.slot_bus.clear();
        p->h.slot_gain.clear();
        p->h.bus_revision++;
        device_console_drop(p->h);  // the console's stages sat behind that table
        return SRACK_OK;
    });
}

int srack_voices_set_field_f32(srack_patch* p, int module, int field, const float* values) { return set_voice_field(p, module, field, values); }
int srack_voices_set_field_f64(srack_patch* p, int module, int field, const double* values) { return set_voice_field(p, module, field, values); }

int srack_render_planes(srack_patch* p, int* channel_plane, int cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        int rc = ensure_program(p->h, p->h.prog_valid ? p->h.prog_flags : 0u);
        if (rc != SRACK_OK) return rc;
        const DevProgram& H = p->h.prog.voice.hdr;
        for (int c = 0; c < H.n_channels && c < cap && channel_plane; c++) channel_plane[c] = H.channel_plane[c];
        return H.n_planes;
    });
}

int srack_render(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix, uint32_t flags, void* stream)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (p->h.n_voices == 0) {
            set_error("render: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        return device_render(p->h, n_samples, d_frames, d_mix, nullptr, nullptr, flags, stream);
    });
}

int srack_render_stats(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix, double* d_stats, uint32_t flags, void* stream)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (((uintptr_t)d_stats & 7u) != 0) {  // (before anything touches the device)
            set_error("render_stats: d_stats must be 8-byte aligned");
            return SRACK_ERR_INVALID;
        }
        if (p->h.n_voices == 0) {
            set_error("render_stats: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        return device_render(p->h, n_samples, d_frames, d_mix, d_stats, nullptr, flags, stream);
    });
}

int srack_voices_set_buses(srack_patch* p, uint32_t n_buses, const int* bus, const float* gain)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        PatchHandle& h = p->h;
        if (h.n_voices == 0) {
            set_error("voices_set_buses: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        if (n_buses == 0 || n_buses > SRACK_MAX_BUSES) {
            set_error("voices_set_buses: n_buses must be 1 .. 65536");
            return SRACK_ERR_INVALID;
        }
        for (uint32_t v = 0; bus && v < h.n_voices; v++)
            if (bus[v] < SRACK_BUS_NONE || (bus[v] >= 0 && (uint32_t)bus[v] >= n_buses)) {
                set_error("voices_set_buses: voice " + std::to_string(v) + " names bus " + std::to_string(bus[v]) + " of " + std::to_string(n_buses));
                return SRACK_ERR_INVALID;
            }
        // (built aside and committed at the end: a failure above or an allocation failure here leaves the old table in place)
        std::vector<int32_t> b(h.n_voices, 0);
        std::vector<float> g(h.n_voices, 1.0f);
        if (bus) std::copy(bus, bus + h.n_voices, b.begin());
        if (gain) std::copy(gain, gain + h.n_voices, g.begin());
        BusPlan plan = bus_plan_make(h.n_voices, n_buses, b.data());
        if (n_buses != h.n_buses) device_console_drop(h);  // other buses: the console's stages go, settings and state (the same count keeps all)
        h.n_buses = n_buses;
        h.bus = std::move(b);
        h.bus_gain = std::move(g);
        h.bus_plan = std::move(plan);
        h.bus_slots = 0;  // (the one table of the handle is of this kind now)
        h.slot_bus.clear();
        h.slot_gain.clear();
        h.bus_revision++;
        return SRACK_OK;
    });
}

int srack_voices_set_bus_slots(srack_patch* p, uint32_t n_buses, uint32_t n_slots, const int* bus, const float* gain)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        PatchHandle& h = p->h;
        if (h.n_voices == 0) {
            set_error("voices_set_bus_slots: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        if (n_buses == 0 || n_buses > SRACK_MAX_BUSES) {
            set_error("voices_set_bus_slots: n_buses must be 1 .. 65536");
            return SRACK_ERR_INVALID;
        }
        if (n_slots == 0 || n_slots > SRACK_MAX_VOICE_SLOTS) {
            set_error("voices_set_bus_slots: n_slots must be 1 .. 4");
            return SRACK_ERR_INVALID;
        }
        const size_t V = h.n_voices, K = n_slots, C = (size_t)h.graph.cfg.channels;
        for (size_t i = 0; bus && i < V * K; i++)
            if (bus[i] < SRACK_BUS_NONE || (bus[i] >= 0 && (uint32_t)bus[i] >= n_buses)) {
                set_error("voices_set_bus_slots: voice " + std::to_string(i / K) + " slot " + std::to_string(i % K) + " names bus " + std::to_string(bus[i]) + " of " + std::to_string(n_buses));
                return SRACK_ERR_INVALID;
            }
        // (built aside and committed at the end, as in srack_voices_set_buses)
        std::vector<int32_t> sb(V * K, SRACK_BUS_NONE), b0(V);
        std::vector<float> sg(V * K * C, 1.0f), g0(V);
        if (bus) std::copy(bus, bus + V * K, sb.begin());
        else
            for (size_t v = 0; v < V; v++) sb[v * K] = 0;
        if (gain) std::copy(gain, gain + V * K * C, sg.begin());
        for (size_t v = 0; v < V; v++) {
            b0[v] = sb[v * K];
            g0[v] = sg[v * K * C];
        }
        BusPlan plan = bus_slot_plan_make(h.n_voices, n_buses, n_slots, sb.data());
        if (n_buses != h.n_buses) device_console_drop(h);
        h.n_buses = n_buses;
        h.bus = std::move(b0);
        h.bus_gain = std::move(g0);
        h.bus_plan = std::move(plan);
        h.bus_slots = n_slots;
        h.slot_bus = std::move(sb);
        h.slot_gain = std::move(sg);
        h.bus_revision++;
        return SRACK_OK;
    });
}

int srack_voices_get_bus_slots(const srack_patch* p, int* n_slots, int* bus, float* gain, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const PatchHandle& h = p->h;
        const size_t K = h.bus_slots ? h.bus_slots : 1u, C = (size_t)h.graph.cfg.channels;
        const size_t n = h.n_buses ? std::min(cap, h.n_voices) : 0u;
        if (n_slots) *n_slots = h.n_buses ? (int)K : 0;
        if (h.bus_slots) {
            if (bus) std::copy(h.slot_bus.begin(), h.slot_bus.begin() + n * K, bus);
            if (gain) std::copy(h.slot_gain.begin(), h.slot_gain.begin() + n * K * C, gain);
        } else {  // a table set through srack_voices_set_buses: one slot, the gain repeated per channel
            if (bus) std::copy(h.bus.begin(), h.bus.begin() + n, bus);
            for (size_t i = 0; gain && i < n * C; i++) gain[i] = h.bus_gain[i / C];
        }
        return (int)h.n_buses;
    });
}

int srack_voices_get_buses(const srack_patch* p, int* bus, float* gain, uint32_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const PatchHandle& h = p->h;
        const uint32_t n = h.n_buses ? std::min(cap, h.n_voices) : 0u;
        if (bus) std::copy(h.bus.begin(), h.bus.begin() + n, bus);
        if (gain) std::copy(h.bus_gain.begin(), h.bus_gain.begin() + n, gain);
        return (int)h.n_buses;
    });
}

int srack_voices_bus_plan(const srack_patch* p, int* segments, uint32_t segment_cap, int* order, uint32_t order_cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        const BusPlan& B = p->h.bus_plan;
        const uint32_t K = p->h.bus_slots ? p->h.bus_slots : 1u;  // a slot table: `i` below is the group tile * K + slot
        uint32_t n_order = 0;
        for (uint32_t i = 0; i < B.n_tiles; i++)
            for (uint32_t s = B.tile_seg[i]; s < B.tile_seg[i + 1]; s++) {
                const uint32_t j0 = s == B.tile_seg[i] ? 0u : B.seg_end[s - 1], j1 = B.seg_end[s];
                if (segments && s < segment_cap) {
                    segments[4 * s + 0] = (int)i;
                    segments[4 * s + 1] = B.seg_bus[s];
                    segments[4 * s + 2] = B.seg_dst[s] >= 0 ? B.seg_dst[s] : -1;
                    segments[4 * s + 3] = (int)(j1 - j0);
                }
                for (uint32_t j = j0; j < j1; j++, n_order++)
                    if (order && n_order < order_cap) order[n_order] = (int)(i / K * kBusTile + B.order[(size_t)i * kBusTile + j]);
            }
        return (int)B.seg_end.size();
    });
}

int srack_render_buses(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix, double* d_stats, float* d_bus_mix, uint32_t flags, void* stream)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (((uintptr_t)d_stats & 7u) != 0) {
            set_error("render_buses: d_stats must be 8-byte aligned");
            return SRACK_ERR_INVALID;
        }
        if (p->h.n_voices == 0) {
            set_error("render_buses: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        if (d_bus_mix && p->h.n_buses == 0) {
            set_error("render_buses: d_bus_mix given and no mix table set: call srack_voices_set_buses first");
            return SRACK_ERR_STATE;
        }
        return device_render(p->h, n_samples, d_frames, d_mix, d_stats, d_bus_mix, flags, stream);
    });
}

// ---- the bus console: what its calls ask of their arguments ------------------------------------------------------
// what every call of every stage asks first
static int console_preamble(const srack_patch* p, const char* who)
{
    CHECK_HANDLE(p);
    const PatchHandle& h = p->h;
    if (h.n_voices == 0) {
        set_error(std::string(who) + ": call srack_voices_configure first");
        return SRACK_ERR_STATE;
    }
    if (h.n_buses == 0) {
        set_error(std::string(who) + ": no mix table set: call srack_voices_set_buses first");
        return SRACK_ERR_STATE;
    }
    return SRACK_OK;
}

// a stage's calls other than its setter and getter: `noun` ("filters") must have been set by srack_buses_set_<setter> ("filter")
static int need_set(bool set, const char* who, const char* noun, const char* setter)
{
    if (set) return SRACK_OK;
    set_error(std::string(who) + ": no " + noun + " set: call srack_buses_set_" + setter + " first");
    return SRACK_ERR_STATE;
}

// the rows a stage reads and the buffer `out` ("d_out", the master's "d_master") it writes
static int need_rows(const char* who, const void* d_rows, const void* d_out, const char* out, uint32_t row_channels)
{
    if (!d_rows || !d_out) {
        set_error(std::string(who) + ": d_rows and " + out + " must be given");
        return SRACK_ERR_INVALID;
    }
    if (row_channels < 1 || row_channels > 8) {
        set_error(std::string(who) + ": row_channels must be 1 .. 8");
        return SRACK_ERR_INVALID;
    }
    return SRACK_OK;
}

// do na bytes at a and nb bytes at b overlap
static bool meet(const void* a, uint64_t na, const void* b, uint64_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }

// a stage that may work in place: its d_out is d_rows itself or disjoint from it
static int need_in_place_or_apart(const char* who, const void* d_rows, const void* d_out, uint64_t bytes)
{
    if (d_rows == d_out || !meet(d_rows, bytes, d_out, bytes)) return SRACK_OK;
    set_error(std::string(who) + ": d_out overlaps d_rows in part: it must be d_rows itself or disjoint from it");
    return SRACK_ERR_INVALID;
}

// the buffers `a` and `b` of a stage, either of which may be absent: "<a> overlaps <b>"
static int need_apart(const char* who, const char* a_name, const void* a, uint64_t na, const char* b_name, const void* b, uint64_t nb)
{
    if (!a || !b || !meet(a, na, b, nb)) return SRACK_OK;
    set_error(std::string(who) + ": " + a_name + " overlaps " + b_name);
    return SRACK_ERR_INVALID;
}

// ---- the bus reverbs ---------------------------------------------------------------------------------------------
static const double kFvDefaults[SRACK_FREEVERB__NFIELDS] = {0.5, 0.0, 1.0, 0.5, 0.5, 0.0};  // FreeverbModule::new (freeverb.rs:36-60), in field order

static int busfx_lines(const srack_patch* p, const char* who, uint32_t len[kFvLines], uint32_t first[kFvLines], uint32_t* total, uint32_t* block)
{
    if (!fv_line_lengths(p->h.graph.cfg.sample_rate, len, first, total)) {
        set_error(std::string(who) + ": a Freeverb needs a sample rate of at least 784 Hz");
        return SRACK_ERR_UNSUPPORTED;
    }
    *block = 256u;
    for (int j = 0; j < kFvLines; j++) *block = std::min(*block, len[j]);
    return SRACK_OK;
}

int srack_buses_set_reverb(srack_patch* p, const double* params, const int* enabled)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_set_reverb");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        BusFx& F = h.console.busfx;
        uint32_t len[kFvLines], first[kFvLines], total = 0, block = 0;
        if ((rc = busfx_lines(p, "buses_set_reverb", len, first, &total, &block)) != SRACK_OK) return rc;
        const size_t n = h.n_buses;
        // (built aside: an allocation failure leaves the earlier setting in place)
        std::vector<double> par(n * SRACK_FREEVERB__NFIELDS);
        std::vector<uint8_t> en(n, 1);
        for (size_t b = 0; b < n; b++) {
            for (int f = 0; f < SRACK_FREEVERB__NFIELDS; f++) par[b * SRACK_FREEVERB__NFIELDS + f] = params ? params[b * SRACK_FREEVERB__NFIELDS + f] : kFvDefaults[f];
            if (enabled) en[b] = enabled[b] != 0;
        }
        if (!F.set) {
            F.d_state.assign(n, nullptr);
            F.fresh.assign(n, 1);
            F.counter = 0;
        }
        for (size_t b = 0; b < n; b++)
            if (F.set && F.enabled[b] && !en[b]) device_busfx_free_bus(h, (uint32_t)b);  // disabling drops the state: enabled again, the bus starts afresh
        std::copy(len, len + kFvLines, F.len);
        std::copy(first, first + kFvLines, F.first);
        F.total = total;
        F.block = block;
        F.params = std::move(par);
        F.enabled = std::move(en);
        F.tab_dirty = true;  // coefficients change, lines and filter states stay: the reference's slider, set_freeverb(false)
        F.set = true;
        return SRACK_OK;
    });
}

int srack_buses_get_reverb(const srack_patch* p, double* params, int* enabled, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_reverb");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const BusFx& F = h.console.busfx;
        if (!F.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (params) std::copy(F.params.begin(), F.params.begin() + n * SRACK_FREEVERB__NFIELDS, params);
        for (size_t b = 0; enabled && b < n; b++) enabled[b] = F.enabled[b];
        return (int)h.n_buses;
    });
}

int srack_buses_reset_reverb(srack_patch* p)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reset_reverb");
        if (rc != SRACK_OK) return rc;
        BusFx& F = p->h.console.busfx;
        if ((rc = need_set(F.set, "buses_reset_reverb", "reverbs", "reverb")) != SRACK_OK) return rc;
        std::fill(F.fresh.begin(), F.fresh.end(), (uint8_t)1);  // zeroed on the next call's stream, before its kernel
        F.counter = 0;
        return SRACK_OK;
    });
}

int srack_buses_reverb_plan(const srack_patch* p, int* line_lengths, int* block)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reverb_plan");
        if (rc != SRACK_OK) return rc;
        uint32_t len[kFvLines], first[kFvLines], total = 0, T = 0;
        if ((rc = busfx_lines(p, "buses_reverb_plan", len, first, &total, &T)) != SRACK_OK) return rc;
        for (int j = 0; line_lengths && j < kFvLines; j++) line_lengths[j] = (int)len[j];
        if (block) *block = (int)T;
        return SRACK_OK;
    });
}

int srack_buses_reverb(srack_patch* p, uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reverb");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busfx.set, "buses_reverb", "reverbs", "reverb")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if (!d_bus_mix || !d_bus_fx) {
            set_error("buses_reverb: d_bus_mix and d_bus_fx must be given");
            return SRACK_ERR_INVALID;
        }
        const uint64_t in_bytes = 4ull * h.n_buses * h.graph.cfg.channels * n_samples, out_bytes = 4ull * h.n_buses * 2 * n_samples;
        if (meet(d_bus_mix, in_bytes, d_bus_fx, out_bytes)) {
            set_error("buses_reverb: d_bus_fx overlaps d_bus_mix");
            return SRACK_ERR_INVALID;
        }
        return device_buses_reverb(h, n_samples, d_bus_mix, d_bus_fx, stream);
    });
}

// ---- the master section ------------------------------------------------------------------------------------------
int srack_buses_set_master(srack_patch* p, const float* gain)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_set_master");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        // (built aside: an allocation failure leaves the earlier gains in place)
        std::vector<float> g((size_t)h.n_buses * 2, 1.0f);
        if (gain) std::memcpy(g.data(), gain, sizeof(float) * g.size());  // (bit for bit: NaN payloads, signed zeros)
        h.console.master.gain = std::move(g);
        h.console.master.set = true;
        device_master_gains_changed(h);
        return SRACK_OK;
    });
}

int srack_buses_get_master(const srack_patch* p, float* gain, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_master");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        if (!h.console.master.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (gain && n) std::memcpy(gain, h.console.master.gain.data(), sizeof(float) * 2 * n);
        return (int)h.n_buses;
    });
}

int srack_buses_master(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_master, double* d_master_stats, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_master");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if (n_samples == 0) return SRACK_OK;
        if ((rc = need_rows("buses_master", d_rows, d_master, "d_master", row_channels)) != SRACK_OK) return rc;
        if (((uintptr_t)d_master_stats & 7u) != 0) {
            set_error("buses_master: d_master_stats must be 8-byte aligned");
            return SRACK_ERR_INVALID;
        }
        if (meet(d_rows, 4ull * h.n_buses * row_channels * n_samples, d_master, 4ull * 2 * n_samples)) {
            set_error("buses_master: d_master overlaps d_rows");
            return SRACK_ERR_INVALID;
        }
        return device_buses_master(h, n_samples, d_rows, row_channels, d_master, d_master_stats, stream);
    });
}

// ---- the bus sends -------------------------------------------------------------------------------------------------
// The host's list laid out for the kernels (sends.hip.h): a stable grouping by destination, the terms in CSR order with every
// destination's through term first, one run per SRACK_MASTER_RUN terms.  A destination of one run is summed straight into its row; the
// runs of any other get scratch rows, side by side, and an entry in the table of the tree kernel.
static void sends_plan_make(Sends& S, uint32_t n_buses)
{
    const size_t n_sends = S.src.size();
    S.n_terms.assign(n_buses, 1);
    for (size_t i = 0; i < n_sends; i++) S.n_terms[S.dst[i]]++;
    std::vector<size_t> first(n_buses + 1, 0);  // a destination's first term
    for (uint32_t d = 0; d < n_buses; d++) first[d + 1] = first[d] + (size_t)S.n_terms[d];
    S.term_src.assign(n_buses + n_sends, 0);
    S.term_gain.assign((n_buses + n_sends) * 2, 0.0f);
    S.order.assign(n_sends, 0);
    std::vector<size_t> fill(n_buses);
    for (uint32_t d = 0; d < n_buses; d++) {
        S.term_src[first[d]] = d;
        std::memcpy(&S.term_gain[first[d] * 2], &S.through[(size_t)d * 2], sizeof(float) * 2);
        fill[d] = first[d] + 1;
    }
    for (size_t i = 0; i < n_sends; i++) {  // (ascending i within a destination: stable)
        const size_t at = fill[S.dst[i]]++;
        S.term_src[at] = (uint32_t)S.src[i];
        std::memcpy(&S.term_gain[at * 2], &S.gain[i * 2], sizeof(float) * 2);
        S.order[at - (size_t)S.dst[i] - 1] = (int32_t)i;  // (d + 1 through terms lie in front of destination d's sends)
    }
    S.runs.clear();
    S.multi.clear();
    S.scratch_rows = 0;
    S.max_blocks = 0;
    for (uint32_t d = 0; d < n_buses; d++) {
        const uint32_t n = (uint32_t)S.n_terms[d], n_runs = (n + SRACK_MASTER_RUN - 1) / SRACK_MASTER_RUN;
        if (n_runs > 1) {
            const uint32_t m[4] = {d, S.scratch_rows, n_runs, 0u};
            S.multi.insert(S.multi.end(), m, m + 4);
            S.max_blocks = std::max(S.max_blocks, (n_runs + SRACK_MASTER_BLOCK - 1) / SRACK_MASTER_BLOCK);
        }
        for (uint32_t r = 0; r < n_runs; r++) {
            const uint32_t run[4] = {d, (uint32_t)first[d] + r * SRACK_MASTER_RUN, std::min<uint32_t>(SRACK_MASTER_RUN, n - r * SRACK_MASTER_RUN),
                                     n_runs > 1 ? S.scratch_rows + r : 0xFFFFFFFFu};
            S.runs.insert(S.runs.end(), run, run + 4);
        }
        if (n_runs > 1) S.scratch_rows += n_runs;
    }
}

int srack_buses_set_sends(srack_patch* p, uint32_t n_sends, const int* src, const int* dst, const float* gain, const float* through)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_set_sends");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if (n_sends > SRACK_MAX_SENDS) {
            set_error("buses_set_sends: n_sends must be at most " + std::to_string(SRACK_MAX_SENDS));
            return SRACK_ERR_INVALID;
        }
        if (n_sends == 0) {  // no sends: none set
            device_sends_drop(h);
            return SRACK_OK;
        }
        if (!src || !dst) {
            set_error("buses_set_sends: src and dst must be given");
            return SRACK_ERR_INVALID;
        }
        std::vector<uint32_t> feeders(h.n_buses, 0);
        for (uint32_t i = 0; i < n_sends; i++) {
            if (src[i] < 0 || (uint32_t)src[i] >= h.n_buses || dst[i] < 0 || (uint32_t)dst[i] >= h.n_buses) {
                set_error("buses_set_sends: send " + std::to_string(i) + " goes from bus " + std::to_string(src[i]) + " to bus " + std::to_string(dst[i]) + " of " +
                          std::to_string(h.n_buses));
                return SRACK_ERR_INVALID;
            }
            if (++feeders[dst[i]] > 65535u) {  // (with the through term: the tree's 16 blocks of 64 runs of 64 terms)
                set_error("buses_set_sends: bus " + std::to_string(dst[i]) + " is the destination of more than 65535 sends");
                return SRACK_ERR_INVALID;
            }
        }
        // (built aside and committed at the end: a failure above or an allocation failure here leaves the earlier sends in place)
        Sends S;
        S.src.assign(src, src + n_sends);
        S.dst.assign(dst, dst + n_sends);
        S.gain.assign((size_t)n_sends * 2, 1.0f);
        S.through.assign((size_t)h.n_buses * 2, 1.0f);
        if (gain) std::memcpy(S.gain.data(), gain, sizeof(float) * S.gain.size());  // (bit for bit: NaN payloads, signed zeros)
        if (through) std::memcpy(S.through.data(), through, sizeof(float) * S.through.size());
        sends_plan_make(S, h.n_buses);
        Sends& T = h.console.sends;  // the device side stays: tables (uploaded again by the next call), scratch, event and note
        T.src = std::move(S.src), T.dst = std::move(S.dst), T.gain = std::move(S.gain), T.through = std::move(S.through);
        T.n_terms = std::move(S.n_terms), T.order = std::move(S.order), T.term_src = std::move(S.term_src), T.term_gain = std::move(S.term_gain);
        T.runs = std::move(S.runs), T.multi = std::move(S.multi);
        T.scratch_rows = S.scratch_rows;
        T.max_blocks = S.max_blocks;
        T.set = true;
        device_sends_changed(h);
        return SRACK_OK;
    });
}

int srack_buses_get_sends(const srack_patch* p, int* src, int* dst, float* gain, uint32_t cap, float* through, uint32_t through_cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_sends");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const Sends& S = h.console.sends;
        if (!S.set) return 0;
        const size_t n = std::min<size_t>(cap, S.src.size()), nb = std::min<size_t>(through_cap, h.n_buses);
        if (src && n) std::memcpy(src, S.src.data(), sizeof(int) * n);
        if (dst && n) std::memcpy(dst, S.dst.data(), sizeof(int) * n);
        if (gain && n) std::memcpy(gain, S.gain.data(), sizeof(float) * 2 * n);
        if (through && nb) std::memcpy(through, S.through.data(), sizeof(float) * 2 * nb);
        return (int)S.src.size();
    });
}

int srack_buses_send_plan(const srack_patch* p, int* n_terms, uint32_t bus_cap, int* order, uint32_t order_cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_send_plan");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const Sends& S = h.console.sends;
        if (!S.set) return 0;
        const size_t nb = std::min<size_t>(bus_cap, h.n_buses), n = std::min<size_t>(order_cap, S.order.size());
        if (n_terms && nb) std::memcpy(n_terms, S.n_terms.data(), sizeof(int) * nb);
        if (order && n) std::memcpy(order, S.order.data(), sizeof(int) * n);
        return (int)(S.runs.size() / 4);
    });
}

int srack_buses_send(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_out, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_send");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.sends.set, "buses_send", "sends", "sends")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if ((rc = need_rows("buses_send", d_rows, d_out, "d_out", row_channels)) != SRACK_OK) return rc;
        const uint64_t bytes = 4ull * h.n_buses * row_channels * n_samples;
        if (meet(d_rows, bytes, d_out, bytes)) {
            set_error("buses_send: d_out overlaps d_rows");
            return SRACK_ERR_INVALID;
        }
        return device_buses_send(h, n_samples, d_rows, row_channels, d_out, stream);
    });
}

// ---- the bus filters -----------------------------------------------------------------------------------------------
static const float kBusVcfDefaults[SRACK_BUS_FILTER_NPARAMS] = {0.2f, 0.5f, 0.5f};  // MoogFilterModule::new: freq, res, exp_amt

int srack_buses_set_filter(srack_patch* p, const float* params, const int* port, const int* enabled)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_set_filter");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        BusVcf& F = h.console.busvcf;
        const size_t n = h.n_buses;
        for (size_t b = 0; port && b < n; b++)
            if (port[b] < SRACK_VCF_OUT_LOWPASS || port[b] > SRACK_VCF_OUT_HIGHPASS) {
                set_error("buses_set_filter: bus " + std::to_string(b) + " asks for port " + std::to_string(port[b]) + ": a filter has outputs 0 .. 2");
                return SRACK_ERR_INVALID;
            }
        // (built aside: a failure leaves the earlier setting in place)
        std::vector<float> par(n * SRACK_BUS_FILTER_NPARAMS);
        std::vector<int32_t> po(n, SRACK_VCF_OUT_LOWPASS);
        std::vector<uint8_t> en(n, 1);
        for (size_t b = 0; b < n; b++) {
            for (int f = 0; f < SRACK_BUS_FILTER_NPARAMS; f++) par[b * SRACK_BUS_FILTER_NPARAMS + f] = kBusVcfDefaults[f];
            if (port) po[b] = port[b];
            if (enabled) en[b] = enabled[b] != 0;
        }
        if (params) std::memcpy(par.data(), params, sizeof(float) * par.size());  // bit for bit
        if ((rc = device_busvcf_enable(h, en)) != SRACK_OK) return rc;  // the state follows its buses: a bus enabled now starts from zeros, a disabled one drops its state
        F.params = std::move(par);
        F.port = std::move(po);
        F.enabled = std::move(en);
        F.set = true;
        device_busvcf_changed(h);  // the sliders: the table is made again, the state stays
        return SRACK_OK;
    });
}

int srack_buses_get_filter(const srack_patch* p, float* params, int* port, int* enabled, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_filter");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const BusVcf& F = h.console.busvcf;
        if (!F.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (params && n) std::memcpy(params, F.params.data(), sizeof(float) * n * SRACK_BUS_FILTER_NPARAMS);
        for (size_t b = 0; port && b < n; b++) port[b] = F.port[b];
        for (size_t b = 0; enabled && b < n; b++) enabled[b] = F.enabled[b];
        return (int)h.n_buses;
    });
}

int srack_buses_reset_filter(srack_patch* p)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reset_filter");
        if (rc != SRACK_OK) return rc;
        if ((rc = need_set(p->h.console.busvcf.set, "buses_reset_filter", "filters", "filter")) != SRACK_OK) return rc;
        device_busvcf_reset(p->h);
        return SRACK_OK;
    });
}

int srack_buses_filter_state(srack_patch* p, float* state, uint32_t cap)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_filter_state");
        if (rc != SRACK_OK) return rc;
        if ((rc = need_set(p->h.console.busvcf.set, "buses_filter_state", "filters", "filter")) != SRACK_OK) return rc;
        if (state && cap && (rc = device_busvcf_state(p->h, state, cap)) != SRACK_OK) return rc;
        return (int)p->h.n_buses;
    });
}

int srack_buses_filter(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_filter");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busvcf.set, "buses_filter", "filters", "filter")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if ((rc = need_rows("buses_filter", d_rows, d_out, "d_out", row_channels)) != SRACK_OK) return rc;
        const uint64_t bytes = 4ull * h.n_buses * row_channels * n_samples, cv_bytes = 4ull * h.n_buses * n_samples;
        if ((rc = need_in_place_or_apart("buses_filter", d_rows, d_out, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_filter", "d_cv", d_cv, cv_bytes, "d_out", d_out, bytes)) != SRACK_OK) return rc;
        return device_buses_filter(h, n_samples, d_rows, row_channels, d_cv, d_out, stream);
    });
}

// ---- the bus VCAs ----------------------------------------------------------------------------------------------------
static const float kBusVcaDefaults[SRACK_BUS_VCA_NPARAMS] = {0.0f, 0.5f, 0.25f, 0.5f};  // ADSRModule::new: a_sec, d_sec, s_val, r_sec

int srack_buses_set_vca(srack_patch* p, const float* params, const int* mode, const int* negative)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_set_vca");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        BusVca& F = h.console.busvca;
        const size_t n = h.n_buses;
        for (size_t b = 0; mode && b < n; b++)
            if (mode[b] < SRACK_BUS_VCA_OFF || mode[b] > SRACK_BUS_VCA_GATE) {
                set_error("buses_set_vca: bus " + std::to_string(b) + " asks for mode " + std::to_string(mode[b]) + ": a bus VCA is off (0), CV (1) or gate (2)");
                return SRACK_ERR_INVALID;
            }
        // (built aside: a failure leaves the earlier setting in place)
        std::vector<float> par(n * SRACK_BUS_VCA_NPARAMS);
        std::vector<int32_t> mo(n, SRACK_BUS_VCA_GATE);
        std::vector<uint8_t> neg(n, 0);
        for (size_t b = 0; b < n; b++) {
            for (int f = 0; f < SRACK_BUS_VCA_NPARAMS; f++) par[b * SRACK_BUS_VCA_NPARAMS + f] = kBusVcaDefaults[f];
            if (mode) mo[b] = mode[b];
            if (negative) neg[b] = negative[b] != 0;
        }
        if (params) std::memcpy(par.data(), params, sizeof(float) * par.size());  // bit for bit
        if ((rc = device_busvca_modes(h, mo)) != SRACK_OK) return rc;  // a bus that becomes GATE starts fresh, one that leaves GATE drops its state
        F.params = std::move(par);
        F.mode = std::move(mo);
        F.negative = std::move(neg);
        F.rate = h.graph.adsr_sample_rate();
        F.set = true;
        device_busvca_changed(h);  // the sliders: the table goes up again, the state stays
        return SRACK_OK;
    });
}

int srack_buses_get_vca(const srack_patch* p, float* params, int* mode, int* negative, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_vca");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const BusVca& F = h.console.busvca;
        if (!F.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (params && n) std::memcpy(params, F.params.data(), sizeof(float) * n * SRACK_BUS_VCA_NPARAMS);
        for (size_t b = 0; mode && b < n; b++) mode[b] = F.mode[b];
        for (size_t b = 0; negative && b < n; b++) negative[b] = F.negative[b];
        return (int)h.n_buses;
    });
}

int srack_buses_reset_vca(srack_patch* p)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reset_vca");
        if (rc != SRACK_OK) return rc;
        if ((rc = need_set(p->h.console.busvca.set, "buses_reset_vca", "VCAs", "vca")) != SRACK_OK) return rc;
        device_busvca_reset(p->h);
        return SRACK_OK;
    });
}

int srack_buses_vca_state(srack_patch* p, float* state, uint32_t cap)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_vca_state");
        if (rc != SRACK_OK) return rc;
        if ((rc = need_set(p->h.console.busvca.set, "buses_vca_state", "VCAs", "vca")) != SRACK_OK) return rc;
        if (state && cap && (rc = device_busvca_state(p->h, state, cap)) != SRACK_OK) return rc;
        return (int)p->h.n_buses;
    });
}

int srack_buses_vca(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_ctl, float* d_out, float* d_env,
                    void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_vca");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busvca.set, "buses_vca", "VCAs", "vca")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if ((rc = need_rows("buses_vca", d_rows, d_out, "d_out", row_channels)) != SRACK_OK) return rc;
        const uint64_t bytes = 4ull * h.n_buses * row_channels * n_samples, row_bytes = 4ull * h.n_buses * n_samples;
        if ((rc = need_in_place_or_apart("buses_vca", d_rows, d_out, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_vca", "d_ctl", d_ctl, row_bytes, "d_out", d_out, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_vca", "d_env", d_env, row_bytes, "d_out", d_out, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_vca", "d_env", d_env, row_bytes, "d_rows", d_rows, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_vca", "d_env", d_env, row_bytes, "d_ctl", d_ctl, row_bytes)) != SRACK_OK) return rc;
        return device_buses_vca(h, n_samples, d_rows, row_channels, d_ctl, d_out, d_env, stream);
    });
}

// ---- the bus oscillators ---------------------------------------------------------------------------------------------
static const float kBusOscDefaults[SRACK_BUS_OSC_NPARAMS] = {0.0f, 1.0f, 0.0f};  // OscillatorModule::new's val; a gain of 1, an offset of 0

int srack_buses_set_osc(srack_patch* p, const float* params, const int* port, const int* antialiasing, const int* enabled)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_set_osc");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        BusOsc& F = h.console.busosc;
        const size_t n = h.n_buses;
        for (size_t b = 0; port && b < n; b++)
            if (port[b] < SRACK_OSC_OUT_SINE || port[b] > SRACK_OSC_OUT_SAW) {
                set_error("buses_set_osc: bus " + std::to_string(b) + " asks for port " + std::to_string(port[b]) + ": an oscillator has sine (0), square (1) and sawtooth (2)");
                return SRACK_ERR_INVALID;
            }
        // (built aside: a failure leaves the earlier setting in place)
        std::vector<float> par(n * SRACK_BUS_OSC_NPARAMS);
        std::vector<int32_t> po(n, SRACK_OSC_OUT_SINE);
        std::vector<uint8_t> aa(n, 1), en(n, 1);
        for (size_t b = 0; b < n; b++) {
            for (int f = 0; f < SRACK_BUS_OSC_NPARAMS; f++) par[b * SRACK_BUS_OSC_NPARAMS + f] = kBusOscDefaults[f];
            if (port) po[b] = port[b];
            if (antialiasing) aa[b] = antialiasing[b] != 0;
            if (enabled) en[b] = enabled[b] != 0;
        }
        if (params) std::memcpy(par.data(), params, sizeof(float) * par.size());  // bit for bit
        if ((rc = device_busosc_enable(h, en)) != SRACK_OK) return rc;  // a bus that becomes enabled starts fresh, one that leaves drops its state
        F.params = std::move(par);
        F.port = std::move(po);
        F.aa = std::move(aa);
        F.enabled = std::move(en);
        F.rate = (double)h.graph.cfg.sample_rate;
        F.set = true;
        device_busosc_changed(h);  // the sliders: the table goes up again, the state stays
        return SRACK_OK;
    });
}

int srack_buses_get_osc(const srack_patch* p, float* params, int* port, int* antialiasing, int* enabled, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_osc");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const BusOsc& F = h.console.busosc;
        if (!F.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (params && n) std::memcpy(params, F.params.data(), sizeof(float) * n * SRACK_BUS_OSC_NPARAMS);
        for (size_t b = 0; port && b < n; b++) port[b] = F.port[b];
        for (size_t b = 0; antialiasing && b < n; b++) antialiasing[b] = F.aa[b];
        for (size_t b = 0; enabled && b < n; b++) enabled[b] = F.enabled[b];
        return (int)h.n_buses;
    });
}

int srack_buses_reset_osc(srack_patch* p, const double* pos)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_reset_osc");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busosc.set, "buses_reset_osc", "oscillators", "osc")) != SRACK_OK) return rc;
        for (size_t b = 0; pos && b < h.n_buses; b++)
            if (!(pos[b] >= 0.0 && pos[b] < 1.0) || std::signbit(pos[b])) {  // (a NaN fails both compares; -0.0 passes them)
                set_error("buses_reset_osc: bus " + std::to_string(b) + " asks for phase " + std::to_string(pos[b]) + ": a phase is in [0, 1), and not -0.0");
                return SRACK_ERR_INVALID;
            }
        device_busosc_reset(h, pos);
        return SRACK_OK;
    });
}

int srack_buses_osc_state(srack_patch* p, double* state, uint32_t cap)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_osc_state");
        if (rc != SRACK_OK) return rc;
        if ((rc = need_set(p->h.console.busosc.set, "buses_osc_state", "oscillators", "osc")) != SRACK_OK) return rc;
        if (state && cap && (rc = device_busosc_state(p->h, state, cap)) != SRACK_OK) return rc;
        return (int)p->h.n_buses;
    });
}

int srack_buses_osc(srack_patch* p, uint32_t n_samples, const float* d_cv, const float* d_sync, float* d_out, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_osc");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busosc.set, "buses_osc", "oscillators", "osc")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if (!d_out) {
            set_error("buses_osc: d_out must be given");
            return SRACK_ERR_INVALID;
        }
        const uint64_t row_bytes = 4ull * h.n_buses * n_samples;
        if ((rc = need_apart("buses_osc", "d_cv", d_cv, row_bytes, "d_out", d_out, row_bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_osc", "d_sync", d_sync, row_bytes, "d_out", d_out, row_bytes)) != SRACK_OK) return rc;
        return device_buses_osc(h, n_samples, d_cv, d_sync, d_out, stream);
    });
}

// ---- the bus shapers -------------------------------------------------------------------------------------------------
static const float kBusShaperDefaults[SRACK_BUS_SHAPER_NPARAMS] = {1.0f, 1.0f, 1.0f};  // pre, exponent (NonLinearModule::new's constant), post

int srack_buses_set_shaper(srack_patch* p, const float* params, const int* mode)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_set_shaper");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        BusShaper& F = h.console.busshaper;
        const size_t n = h.n_buses;
        for (size_t b = 0; mode && b < n; b++)
            if (mode[b] < SRACK_BUS_SHAPER_OFF || mode[b] > SRACK_BUS_SHAPER_CV) {
                set_error("buses_set_shaper: bus " + std::to_string(b) + " asks for mode " + std::to_string(mode[b]) + ": a bus shaper is off (0), constant (1) or CV (2)");
                return SRACK_ERR_INVALID;
            }
        // (built aside: a failure leaves the earlier setting in place)
        std::vector<float> par(n * SRACK_BUS_SHAPER_NPARAMS);
        std::vector<int32_t> mo(n, SRACK_BUS_SHAPER_CONST);
        for (size_t b = 0; b < n; b++) {
            for (int f = 0; f < SRACK_BUS_SHAPER_NPARAMS; f++) par[b * SRACK_BUS_SHAPER_NPARAMS + f] = kBusShaperDefaults[f];
            if (mode) mo[b] = mode[b];
        }
        if (params) std::memcpy(par.data(), params, sizeof(float) * par.size());  // bit for bit
        F.params = std::move(par);
        F.mode = std::move(mo);
        F.set = true;
        device_busshaper_changed(h);  // the table goes up again before the next call's kernel
        return SRACK_OK;
    });
}

int srack_buses_get_shaper(const srack_patch* p, float* params, int* mode, uint32_t cap)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_get_shaper");
        if (rc != SRACK_OK) return rc;
        const PatchHandle& h = p->h;
        const BusShaper& F = h.console.busshaper;
        if (!F.set) return 0;
        const size_t n = std::min<size_t>(cap, h.n_buses);
        if (params && n) std::memcpy(params, F.params.data(), sizeof(float) * n * SRACK_BUS_SHAPER_NPARAMS);
        for (size_t b = 0; mode && b < n; b++) mode[b] = F.mode[b];
        return (int)h.n_buses;
    });
}

int srack_buses_shaper(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream)
{
    return guarded([&]() -> int {
        int rc = console_preamble(p, "buses_shaper");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if ((rc = need_set(h.console.busshaper.set, "buses_shaper", "shapers", "shaper")) != SRACK_OK) return rc;
        if (n_samples == 0) return SRACK_OK;
        if ((rc = need_rows("buses_shaper", d_rows, d_out, "d_out", row_channels)) != SRACK_OK) return rc;
        const uint64_t bytes = 4ull * h.n_buses * row_channels * n_samples, cv_bytes = 4ull * h.n_buses * n_samples;
        if ((rc = need_in_place_or_apart("buses_shaper", d_rows, d_out, bytes)) != SRACK_OK) return rc;
        if ((rc = need_apart("buses_shaper", "d_cv", d_cv, cv_bytes, "d_out", d_out, bytes)) != SRACK_OK) return rc;
        return device_buses_shaper(h, n_samples, d_rows, row_channels, d_cv, d_out, stream);
    });
}

// ---- the bus meters --------------------------------------------------------------------------------------------------
int srack_buses_meter(srack_patch* p, uint64_t first_sample, uint32_t n_samples, const float* d_rows, uint32_t row_channels, uint32_t window,
                      double* d_levels, uint32_t n_windows, double* d_totals, void* stream)
{
    return guarded([&]() -> int {
        const int rc = console_preamble(p, "buses_meter");
        if (rc != SRACK_OK) return rc;
        PatchHandle& h = p->h;
        if (n_samples == 0) return SRACK_OK;
        auto bad = [](const char* what) {
            set_error(std::string("buses_meter: ") + what);
            return SRACK_ERR_INVALID;
        };
        if (!d_rows) return bad("d_rows must be given");
        if (row_channels < 1 || row_channels > 8) return bad("row_channels must be 1 .. 8");
        if (!d_levels && !d_totals) return bad("d_levels or d_totals must be given");
        if (((uintptr_t)d_levels & 7u) != 0) return bad("d_levels must be 8-byte aligned");
        if (((uintptr_t)d_totals & 7u) != 0) return bad("d_totals must be 8-byte aligned");
        if (d_levels) {
            if (window < SRACK_BUS_METER_MIN_WINDOW) return bad("window must be at least SRACK_BUS_METER_MIN_WINDOW (64) samples");
            if (n_windows == 0) return bad("n_windows must be at least 1");
            // (n_windows * window < 2^64; the sum is taken apart so that a first_sample near 2^64 cannot wrap)
            const uint64_t span = (uint64_t)n_windows * window;
            if (first_sample > span || n_samples > span - first_sample) return bad("first_sample + n_samples exceeds n_windows * window");
        }
        const uint64_t row_bytes = 4ull * h.n_buses * row_channels * n_samples, total_bytes = 8ull * SRACK_STAT_COUNT * h.n_buses * 2;
        const uint64_t level_bytes = total_bytes * n_windows;
        if (d_levels && meet(d_levels, level_bytes, d_rows, row_bytes)) return bad("d_levels overlaps d_rows");
        if (d_totals && meet(d_totals, total_bytes, d_rows, row_bytes)) return bad("d_totals overlaps d_rows");
        if (d_levels && d_totals && meet(d_levels, level_bytes, d_totals, total_bytes)) return bad("d_levels overlaps d_totals");
        return device_buses_meter(h, first_sample, n_samples, d_rows, row_channels, window, d_levels, n_windows, d_totals, stream);
    });
}

int srack_render_reserve(srack_patch* p, uint32_t n_samples, int want_mix, uint32_t flags)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (p->h.n_voices == 0) {
            set_error("render_reserve: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        return device_reserve(p->h, n_samples, want_mix != 0, flags);
    });
}

// Every SRACK_* variable of the environment that the library's tuning knobs read (tools/: chunk lengths, generator experiments ...): a host
// process that carries one renders with other kernels than the ones measured and tested — srack_render_info says so (" knobs=[...]"),
// and the parity suites refuse to run with any set (tests/conftest.py).  Not listed: where the kernel cache lives and how much it keeps.
extern char** environ;
static std::string tuning_knobs_note()
{
    std::string s;
    for (char** e = environ; e && *e; e++) {
        if (std::strncmp(*e, "SRACK_", 6) != 0) continue;
        if (std::strncmp(*e, "SRACK_KERNEL_CACHE_", 19) == 0 || std::strncmp(*e, "SRACK_BENCH_", 12) == 0 || std::strncmp(*e, "SRACK_TEST_", 11) == 0) continue;
        s += s.empty() ? " knobs=[" : " ";
        s += *e;
    }
    if (!s.empty()) s += "]";
    return s;
}

int srack_render_info(srack_patch* p, char* buf, size_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        int rc = ensure_program(p->h, p->h.prog_valid ? p->h.prog_flags : 0u);
        if (rc != SRACK_OK) return rc;
        std::string s = p->h.prog.description;
        s += tuning_knobs_note();
        const char* k = device_kernel_name(p->h);
        // (the kernel's name stays LAST: hosts and tests read it with split("kernel="))
        s += device_bus_note(p->h);
        s += device_console_note(p->h);
        s += device_waves_note(p->h);
        s += device_sequences_note(p->h);
        s += device_jit_note(p->h);
        if (k && *k) s += std::string(" kernel=") + k;
        if (buf && cap) {
            std::strncpy(buf, s.c_str(), cap - 1);
            buf[cap - 1] = 0;
        }
        return (int)s.size();
    });
}

int srack_render_kernel_source(srack_patch* p, uint32_t flags, char* buf, size_t cap)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (p->h.n_voices == 0) {
            set_error("render_kernel_source: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        FlatPair scratch;
        const FlatPair* prog = nullptr;
        int rc = peek_program(p->h, flags, scratch, &prog);
        if (rc != SRACK_OK) return rc;
        std::string src;
        rc = jit_source(*prog, 3, jit_ctl_supported(*prog), src);
        if (rc != SRACK_OK) return rc;
        src = "// for: " + prog->description + "\n" + src;  // (for the reader; not part of what is compiled and cached)
        if (buf && cap) {
            std::strncpy(buf, src.c_str(), cap - 1);
            buf[cap - 1] = 0;
        }
        return (int)src.size();
    });
}

int srack_render_kernel_compile(srack_patch* p, uint32_t flags)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        if (p->h.n_voices == 0) {
            set_error("render_kernel_compile: call srack_voices_configure first");
            return SRACK_ERR_STATE;
        }
        FlatPair scratch;
        const FlatPair* prog = nullptr;
        int rc = peek_program(p->h, flags, scratch, &prog);
        if (rc != SRACK_OK) return rc;
        return jit_compile_only(*prog, 3, jit_ctl_supported(*prog));
    });
}

int srack_render_kernel_ms(srack_patch* p, double* avg_ms, int* n_launches, int reset)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        return device_kernel_ms(p->h, avg_ms, n_launches, reset);
    });
}

int srack_voices_get_field(srack_patch* p, int module, int field, double* values)
{
    return guarded([&]() -> int {
        CHECK_HANDLE(p);
        PatchHandle& h = p->h;
        if (!values || h.n_voices == 0) {
            set_error("voices_get_field: bad arguments / voices not configured");
            return SRACK_ERR_INVALID;
        }
        int rc = ensure_program(h, h.prog_valid ? h.prog_flags : 0u);
        if (rc != SRACK_OK) return rc;
        {  // (before anything looks the field up in the device tables: a field the module does not have has no row there)
            const int nf = h.graph.num_fields(module);
            if (nf < 0 || field < 0 || field >= nf) {
                set_error("voices_get_field: no such module/field");
                return SRACK_ERR_INVALID;
            }
        }
        std::vector<double> got;
        if (read_device_state(h, module, field, got)) {
            for (uint32_t v = 0; v < h.n_voices; v++) values[v] = got[v];
            return SRACK_OK;
        }
        // a parameter, or a module that is not evaluated: the field value itself
        double x;
        rc = h.graph.get_field(module, field, &x);
        if (rc != SRACK_OK) return rc;
        for (uint32_t v = 0; v < h.n_voices; v++) values[v] = x;
        for (const auto& o : h.overrides)
            if (o.module == module && o.field == field)
                for (uint32_t v = 0; v < h.n_voices; v++) values[v] = o.values[v];
        return SRACK_OK;
    });
}

extern "C++" {
namespace srack {
bool read_device_state(PatchHandle& h, int module, int field, std::vector<double>& values)
{
    if (!h.prog_valid || !h.dev || module < 0 || module >= (int)h.graph.modules.size()) return false;
    // a module evaluated by the control program has ONE state, shared by every voice
    const int stage = h.prog.n_tracks > 0 && module < (int)h.prog.ctl_stage.size() ? h.prog.ctl_stage[(size_t)module] : -1;
    const bool ctl = stage >= 0;
    const FlatProgram& P = ctl ? h.prog.ctl[(size_t)stage] : h.prog.voice;
    const StateLoc loc = P.locate(h.graph, module, field);
    if (loc.row < 0) return false;
    const uint32_t V = P.n_voices;
    std::vector<uint32_t> rows((size_t)V * (loc.f64 ? 2 : 1));
    if (device_read_rows(h, stage, loc.row, loc.f64 ? 2 : 1, rows.data()) != SRACK_OK) return false;
    values.resize(h.n_voices);
    for (uint32_t v = 0; v < h.n_voices; v++) {
        const uint32_t sv = ctl ? 0u : v;
        if (loc.f64) {
            uint64_t u = (uint64_t)rows[sv] | ((uint64_t)rows[(size_t)V + sv] << 32);
            if (loc.fixed64)
                values[v] = std::ldexp((double)u, -64);  // phase * 2^64 (the fused kernel's fixed-point oscillator)
            else
                std::memcpy(&values[v], &u, 8);
        } else if (loc.flag) {
            values[v] = (double)(int32_t)rows[sv];
        } else {
            float f;
            std::memcpy(&f, &rows[sv], 4);
            values[v] = (double)f;
        }
    }
    return true;
}
}  // namespace srack
}  // extern "C++"

// ---- the kernel cache (jit.cpp) ---------------------------------------------------------------------
int srack_kernel_cache_set_dir(const char* dir)
{
    return guarded([&]() -> int { return jit_cache_set_dir(dir); });
}

int srack_kernel_cache_stats(srack_kernel_cache_info* out)
{
    return guarded([&]() -> int {
        if (!out) {
            set_error("srack_kernel_cache_stats: out is null");
            return SRACK_ERR_INVALID;
        }
        const JitCacheStats st = jit_cache_stats();
        std::memset(out, 0, sizeof *out);
        out->compiled = st.compiled;
        out->disk_hits = st.disk_hits;
        out->memory_hits = st.memory_hits;
        out->modules_loaded = st.modules_loaded;
        out->code_evictions = st.code_evictions;
        out->module_evictions = st.module_evictions;
        out->resident_code_objects = st.resident_code_objects;
        out->resident_modules = st.resident_modules;
        out->compile_ms = st.compile_ms;
        std::snprintf(out->directory, sizeof out->directory, "%s", st.directory);
        return SRACK_OK;
    });
}

// ---- device helpers -------------------------------------------------------------------------------
int srack_device_count(int* n)
{
    return guarded([&]() -> int {
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess) c = 0;
        if (n) *n = c;
        return SRACK_OK;
    });
}

int srack_device_set(int device)
{
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(device));
        return SRACK_OK;
    });
}

int srack_device_get(int* device, char* pci_bus_id, size_t cap)
{
    return guarded([&]() -> int {
        int dev = -1;
        HIP_TRY(hipGetDevice(&dev));
        if (device) *device = dev;
        if (pci_bus_id && cap > 0) {
            pci_bus_id[0] = 0;
            HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, (int)std::min<size_t>(cap, 1u << 20), dev));
        }
        return SRACK_OK;
    });
}

int srack_device_alloc(void** d_ptr, size_t bytes)
{
    return guarded([&]() -> int {
        if (!d_ptr) return SRACK_ERR_INVALID;
        HIP_TRY(hipMalloc(d_ptr, bytes));
#if defined(SRK_POISON) && SRK_POISON
        HIP_TRY(hipMemset(*d_ptr, 0xff, bytes));
#endif
        return SRACK_OK;
    });
}

int srack_device_free(void* d_ptr)
{
    return guarded([&]() -> int {
        HIP_TRY(hipFree(d_ptr));
        return SRACK_OK;
    });
}

// Device -> host through PINNED bounce buffers of the library's own, a chunk at a time (DMA into pinned memory, then a CPU copy).  A plain
// hipMemcpyAsync into the caller's pageable memory FOLLOWED BY hipStreamSynchronize on the same stream is what this was until round 5 — and
// what that round's soaks caught losing data: with sixteen processes on one device, one read-back in a few thousand came back with a stretch
// of ZEROS (tens of pages, the same offsets in call after call of one process) where a second read-back of the very same device bytes had the
// data (tools/fuzz_soak_default.py, SOAK_RETRY=2; notes/r05.md R5.2).  It was not a copy the host read too early — the synchronize was there,
// on the copy's own stream, before the call returned (git show 0c84165^:s-rack_amd/csrc/capi.cpp) —: the runtime's staged copy into pageable
// pages itself dropped them.  The caller's pages are never handed to the copy engine now.
//   * per DEVICE a small pool of bounce sets (two pinned halves of kBounceBytes, a non-blocking stream, two events), created on demand and
//     freed when the library is unloaded; no lock is held across a copy (a set is taken out of the pool for the duration);
//   * the copy of chunk k + 1 runs (DMA) under the CPU's memcpy of chunk k;
//   * a large read-back is cut into slices that helper threads copy side by side, each through a set of its own: one core's memcpy into
//     fresh pageable memory (page faults included) is a few GB/s, PCIe is tens.
// Ordering: everything enqueued on `stream` before the call is waited for first (hipStreamSynchronize), as before.
namespace {
constexpr size_t kBounceBytes = size_t(8) << 20;
constexpr size_t kSliceMin = size_t(64) << 20;   // a helper thread is worth it from here
constexpr int kMaxHelpers = 8;
struct BounceSet {
    int device = -1;
    void* half[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
};
struct BouncePool {
    std::mutex m;
    std::vector<BounceSet*> idle;
    ~BouncePool()
    {   // library unload / process exit: the HIP runtime may already be gone — errors are ignored
        for (BounceSet* b : idle) drop(b);
    }
    int take(int device, BounceSet** out)
    {
        {
            std::lock_guard<std::mutex> lock(m);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i]->device == device) {
                    *out = idle[i];
                    idle.erase(idle.begin() + (long)i);
                    return SRACK_OK;
                }
        }
        BounceSet* b = new BounceSet();
        b->device = device;
        auto build = [&]() -> int {
            for (int k = 0; k < 2; k++) {
                HIP_TRY(hipHostMalloc(&b->half[k], kBounceBytes, hipHostMallocDefault));
                HIP_TRY(hipEventCreateWithFlags(&b->done[k], hipEventDisableTiming));
            }
            HIP_TRY(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
            return SRACK_OK;
        };
        const int rc = build();
        if (rc != SRACK_OK) {  // a half-built set never reaches the pool (the error text stays the failing call's)
            drop(b);
            return rc;
        }
        *out = b;
        return SRACK_OK;
    }
    static void drop(BounceSet* b)
    {
        for (int k = 0; k < 2; k++) {
            if (b->half[k]) (void)hipHostFree(b->half[k]);
            if (b->done[k]) (void)hipEventDestroy(b->done[k]);
        }
        if (b->st) (void)hipStreamDestroy(b->st);
        delete b;
    }
    void give(BounceSet* b)
    {
        if (!b) return;
        std::lock_guard<std::mutex> lock(m);
        idle.push_back(b);
    }
};
BouncePool g_bounce_pool;

// one slice, through one set: DMA of chunk k + 1 under the memcpy of chunk k
int bounce_copy(int device, char* dst, const char* src, size_t bytes)
{
    HIP_TRY(hipSetDevice(device));  // (helper threads start on device 0)
    BounceSet* b = nullptr;
    int rc = g_bounce_pool.take(device, &b);
    auto run = [&]() -> int {
        if (rc != SRACK_OK) return rc;
        const size_t n_chunks = (bytes + kBounceBytes - 1) / kBounceBytes;
        auto len = [&](size_t k) { return std::min(kBounceBytes, bytes - k * kBounceBytes); };
        auto issue = [&](size_t k) -> int {
            HIP_TRY(hipMemcpyAsync(b->half[k & 1], src + k * kBounceBytes, len(k), hipMemcpyDeviceToHost, b->st));
            HIP_TRY(hipEventRecord(b->done[k & 1], b->st));
            return SRACK_OK;
        };
        int r = issue(0);
        for (size_t k = 0; k < n_chunks && r == SRACK_OK; k++) {
            if (k + 1 < n_chunks) r = issue(k + 1);  // (its half was emptied by the memcpy of chunk k - 1)
            if (r != SRACK_OK) break;
            HIP_TRY(hipEventSynchronize(b->done[k & 1]));
            std::memcpy(dst + k * kBounceBytes, b->half[k & 1], len(k));
        }
        if (r != SRACK_OK) (void)hipStreamSynchronize(b->st);  // nothing of ours in flight when the set goes back
        return r;
    };
    rc = run();
    g_bounce_pool.give(b);
    return rc;
}
}  // namespace
int srack_device_from_host(void* d_dst, const void* h_src, size_t bytes, void* stream)
{
    return guarded([&]() -> int {
        if (bytes == 0) return SRACK_OK;
        if (!d_dst || !h_src) return SRACK_ERR_INVALID;
        HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the host's memory may be pageable and reused as soon as this returns
        return SRACK_OK;
    });
}

int srack_device_to_host(void* h_dst, const void* d_src, size_t bytes, void* stream)
{
    return guarded([&]() -> int {
        if (bytes == 0) return SRACK_OK;
        if (!h_dst || !d_src) return SRACK_ERR_INVALID;
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // what the caller enqueued before the copy
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const int helpers = (int)std::min<size_t>({(size_t)kMaxHelpers, (size_t)hw, bytes / kSliceMin});
        if (helpers <= 1) return bounce_copy(device, (char*)h_dst, (const char*)d_src, bytes);
        // slices of whole chunks, one helper thread each (the calling thread takes the first)
        const size_t n_chunks = (bytes + kBounceBytes - 1) / kBounceBytes, per = (n_chunks + (size_t)helpers - 1) / (size_t)helpers * kBounceBytes;
        std::vector<int> rcs((size_t)helpers, SRACK_OK);
        std::vector<std::string> errs((size_t)helpers);
        std::vector<std::thread> threads;
        auto slice = [&](int i) {
            const size_t off = (size_t)i * per;
            if (off >= bytes) return;
            rcs[(size_t)i] = guarded([&]() { return bounce_copy(device, (char*)h_dst + off, (const char*)d_src + off, std::min(per, bytes - off)); });
            if (rcs[(size_t)i] != SRACK_OK) errs[(size_t)i] = srack_last_error();  // (thread-local: carried back to the caller's thread below)
        };
        int started = 1;  // (slice 0 is the caller's)
        try {
            for (; started < helpers; started++) threads.emplace_back(slice, started);
        } catch (const std::exception&) {  // no more threads to be had: the slices without one are copied here, after the caller's own
        }
        slice(0);
        for (int i = started; i < helpers; i++) slice(i);
        for (std::thread& t : threads) t.join();
        for (int i = 0; i < helpers; i++)
            if (rcs[(size_t)i] != SRACK_OK) {
                if (i > 0) set_error(errs[(size_t)i]);
                return rcs[(size_t)i];
            }
        return SRACK_OK;
    });
}

int srack_device_sync(void* stream)
{
    return guarded([&]() -> int {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return SRACK_OK;
    });
}

}  // extern "C"
