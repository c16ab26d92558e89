// console.cpp — the host side of the bus console (console.hpp): what one call of each stage enqueues, the stages' device memory and
// their state between calls.  The kernels are units of their own, reached through launch.hpp: this file sees none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "freeverb_params.hpp"
#include "launch.hpp"
#include "runtime.hpp"

namespace srack {

// ---- the stream contract, for every stage ---------------------------------------------------------------------------------------------
int StageSync::begin(void* stream)
{
    if (!ev_done) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev_done = e;
    } else {
        HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev_done, 0));  // (calls may come on different streams: the stage's memory is one)
    }
    return SRACK_OK;
}

int StageSync::end(void* stream)
{
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord((hipEvent_t)ev_done, (hipStream_t)stream));
    return SRACK_OK;
}

void StageSync::wait()
{
    if (ev_done) (void)hipEventSynchronize((hipEvent_t)ev_done);
}

void StageSync::destroy()
{
    if (ev_done) (void)hipEventDestroy((hipEvent_t)ev_done);
    ev_done = nullptr;
}

int DeviceBuf::grow(StageSync& sync, size_t want, const char* who, const char* what)
{
    if (want <= bytes) return SRACK_OK;
    void* fresh = nullptr;
    if (hipMalloc(&fresh, want) != hipSuccess) {
        (void)hipGetLastError();
        set_error(std::string(who) + ": out of device memory for " + what + " (" + std::to_string(want) + " bytes)");
        return SRACK_ERR_NOMEM;
    }
    sync.wait();  // the last call's kernels may still be using the old one
    if (p) (void)hipFree(p);
    p = fresh;
    bytes = want;
    return SRACK_OK;
}

void DeviceBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

// A stage's device memory and its event, once no call uses them any more; the stage is as it was before it was set.
template <class Stage>
static void stage_drop(Stage& F, std::initializer_list<DeviceBuf*> bufs)
{
    F.sync.wait();
    for (DeviceBuf* b : bufs) b->release();
    F.sync.destroy();
    F = Stage();
}

// ---- state by bus, for the stages that keep it that way (the VCAs, the oscillators) ---------------------------------------------------
template <class T, int kFields>
std::vector<T> BusState<T, kFields>::filled(const Fresh& one, size_t n)
{
    std::vector<T> s((size_t)kFields * n);
    for (int f = 0; f < kFields; f++) std::fill(s.begin() + (size_t)f * n, s.begin() + (size_t)(f + 1) * n, one[f]);
    return s;
}

template <class T, int kFields>
void BusState<T, kFields>::reset()
{
    pending.clear();
    fresh = true;  // uploaded before the next call's kernel
}

template <class T, int kFields>
int BusState<T, kFields>::fetch(StageSync& sync, const Fresh& one, size_t n, std::vector<T>& out)
{
    if (!pending.empty()) {
        out = pending;
        return SRACK_OK;
    }
    out = filled(one, n);
    if (all_fresh()) return SRACK_OK;
    sync.wait();
    HIP_TRY(hipMemcpy(out.data(), d_state.p, sizeof(T) * out.size(), hipMemcpyDeviceToHost));
    return SRACK_OK;
}

template <class T, int kFields>
template <class Owns, class WillOwn>
int BusState<T, kFields>::refresh(StageSync& sync, const Fresh& one, size_t n, Owns owns, WillOwn will_own)
{
    if (all_fresh()) return SRACK_OK;  // fresh stays fresh
    bool moved = false;
    for (size_t b = 0; b < n; b++) moved = moved || (owns(b) != will_own(b));
    if (!moved) return SRACK_OK;
    std::vector<T> cur;
    const int rc = fetch(sync, one, n, cur);
    if (rc != SRACK_OK) return rc;
    for (size_t b = 0; b < n; b++)
        if (!owns(b) || !will_own(b))
            for (int f = 0; f < kFields; f++) cur[(size_t)f * n + b] = one[f];
    pending = std::move(cur);
    return SRACK_OK;
}

template <class T, int kFields>
int BusState<T, kFields>::alloc(StageSync& sync, size_t n, const char* who, const char* what)
{
    const int rc = d_state.grow(sync, sizeof(T) * kFields * n, who, what);
    if (rc == SRACK_OK && pending.empty()) fresh = true;
    return rc;
}

template <class T, int kFields>
int BusState<T, kFields>::upload(StageSync& sync, const Fresh& one, size_t n)
{
    if (pending.empty() && !fresh) return SRACK_OK;
    const std::vector<T> up = pending.empty() ? filled(one, n) : pending;
    sync.wait();
    HIP_TRY(hipMemcpy(d_state.p, up.data(), sizeof(T) * kFields * n, hipMemcpyHostToDevice));
    pending.clear();
    fresh = false;
    return SRACK_OK;
}

template <class T, int kFields>
template <class Owns>
int BusState<T, kFields>::hand_out(StageSync& sync, const Fresh& one, size_t n_buses, Owns owns, T* state, uint32_t cap)
{
    std::vector<T> cur;
    const int rc = fetch(sync, one, n_buses, cur);
    if (rc != SRACK_OK) return rc;
    const size_t n = std::min<size_t>(cap, n_buses);
    for (size_t b = 0; b < n; b++)
        for (int f = 0; f < kFields; f++) state[b * kFields + f] = owns(b) ? cur[(size_t)f * n_buses + b] : one[f];
    return SRACK_OK;
}

// ---- the bus reverbs (busfx.hip.h, launched through launch_bus_reverb) ----------------------------------------------------------------
// One workgroup per bus.  The state of an enabled bus is allocated on first use and zeroed on the call's stream; the table of the
// buses (state pointer, derived doubles) is rewritten only after a change of parameters — behind a host-side wait for the last call's
// kernel, which may still be reading it —, so a tick session of unchanged reverbs is one launch and one event per call.
void device_busfx_free_bus(PatchHandle& h, uint32_t bus)
{
    BusFx& F = h.console.busfx;
    if (bus >= F.d_state.size() || !F.d_state[bus]) return;
    F.sync.wait();
    (void)hipFree(F.d_state[bus]);
    F.d_state[bus] = nullptr;
    F.tab_dirty = true;
}

static void busfx_drop(BusFx& F)
{
    F.sync.wait();
    for (double* p : F.d_state)
        if (p) (void)hipFree(p);
    F.d_tab.release();
    F.sync.destroy();
    F = BusFx();
}

int device_buses_reverb(PatchHandle& h, uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream)
{
    BusFx& F = h.console.busfx;
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t n_buses = h.n_buses;
    int rc;
    if ((rc = F.sync.begin(stream)) != SRACK_OK) return rc;
    const size_t state_bytes = sizeof(double) * ((size_t)kFvStates + F.total);
    uint32_t n_enabled = 0;
    for (uint32_t b = 0; b < n_buses; b++) {
        if (!F.enabled[b]) continue;
        n_enabled++;
        if (!F.d_state[b]) {
            void* p = nullptr;
            if (hipMalloc(&p, state_bytes) != hipSuccess) {
                (void)hipGetLastError();
                set_error("buses_reverb: out of device memory for the state of bus " + std::to_string(b) + " (" + std::to_string(state_bytes) + " bytes per enabled bus)");
                return SRACK_ERR_NOMEM;
            }
            F.d_state[b] = (double*)p;
            F.fresh[b] = 1;
            F.tab_dirty = true;
        }
        if (F.fresh[b]) {  // DelayLine::new is vec![0.0; n], filter_state 0.0
            HIP_TRY(hipMemsetAsync(F.d_state[b], 0, state_bytes, st));
            F.fresh[b] = 0;
        }
    }
    if (F.tab_dirty || !F.d_tab.p) {
        std::vector<BusFxDev> tab(n_buses);
        for (uint32_t b = 0; b < n_buses; b++) {
            tab[b].state = F.enabled[b] ? F.d_state[b] : nullptr;
            fv_derive(&F.params[(size_t)b * SRACK_FREEVERB__NFIELDS], tab[b].par);
        }
        if ((rc = F.d_tab.grow(F.sync, sizeof(BusFxDev) * n_buses, "buses_reverb", "the table of the buses")) != SRACK_OK) return rc;
        F.sync.wait();
        HIP_TRY(hipMemcpy(F.d_tab.p, tab.data(), sizeof(BusFxDev) * n_buses, hipMemcpyHostToDevice));
        F.tab_dirty = false;
    }
    BusFxArgs a;
    a.in = d_bus_mix;
    a.out = d_bus_fx;
    a.tab = (const BusFxDev*)F.d_tab.p;
    a.n = n_samples;
    a.channels = h.graph.cfg.channels;
    a.block = F.block;
    for (int j = 0; j < kFvLines; j++) {
        a.len[j] = F.len[j];
        a.first[j] = F.first[j];
        a.pos[j] = (uint32_t)(F.counter % F.len[j]);
    }
    launch_bus_reverb(a, n_buses, st);
    if ((rc = F.sync.end(stream)) != SRACK_OK) return rc;
    F.counter += n_samples;
    F.last_enabled = n_enabled;
    F.last_block = F.block;
    F.ran = true;
    return SRACK_OK;
}

static std::string busfx_note(const BusFx& F)
{
    return F.ran ? " busfx=" + std::to_string(F.last_enabled) + "[block " + std::to_string(F.last_block) + "]" : std::string();
}

// ---- the master section (master.hip.h, launched through launch_master) -------------------------------------------------------------
// Gains on the device, uploaded again after a change — behind a host-side wait for the last call's kernels, which may still be reading
// them —, and the run sums' scratch, grown on demand.  A tick session of unchanged gains and call lengths is the launches and one
// event per call.
void device_master_gains_changed(PatchHandle& h) { h.console.master.gain_dirty = true; }

int device_buses_master(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_master, double* d_master_stats, void* stream)
{
    Master& M = h.console.master;
    const uint32_t n_buses = h.n_buses;
    const uint32_t n_runs = (n_buses + SRACK_MASTER_RUN - 1) / SRACK_MASTER_RUN;
    int rc;
    if ((rc = M.sync.begin(stream)) != SRACK_OK) return rc;
    if ((rc = M.d_runs.grow(M.sync, sizeof(float) * n_runs * 2 * n_samples, "buses_master", "the run sums")) != SRACK_OK) return rc;
    if (M.gain_dirty || !M.d_gain.p) {
        if ((rc = M.d_gain.grow(M.sync, sizeof(float) * 2 * n_buses, "buses_master", "the gains")) != SRACK_OK) return rc;
        M.sync.wait();
        const std::vector<float> ones(M.set ? 0 : (size_t)2 * n_buses, 1.0f);
        HIP_TRY(hipMemcpy(M.d_gain.p, M.set ? M.gain.data() : ones.data(), sizeof(float) * 2 * n_buses, hipMemcpyHostToDevice));
        M.gain_dirty = false;
    }
    MasterArgs a;
    a.rows = d_rows;
    a.gain = (const float*)M.d_gain.p;
    a.runs = (float*)M.d_runs.p;
    a.master = d_master;
    a.stats = d_master_stats;
    a.n = n_samples;
    a.n_buses = n_buses;
    a.row_channels = row_channels;
    a.used = row_channels < 2 ? row_channels : 2u;
    launch_master(a, (hipStream_t)stream);
    if ((rc = M.sync.end(stream)) != SRACK_OK) return rc;
    M.last_buses = n_buses;
    M.ran = true;
    return SRACK_OK;
}

static std::string master_note(const Master& M)
{
    if (!M.ran) return std::string();
    const uint32_t n_runs = (M.last_buses + SRACK_MASTER_RUN - 1) / SRACK_MASTER_RUN;
    return " master=" + std::to_string(M.last_buses) + "[" + std::to_string(n_runs) + " runs]";
}

// ---- the bus sends (sends.hip.h, launched through launch_sends) ----------------------------------------------------------------------
// The tables of the plan on the device in one allocation, uploaded again after a change — behind a host-side wait for the last call's
// kernels, which may still be reading them —, and the scratch for the run sums of the destinations of several runs, grown on demand.
// A tick session of an unchanged list and call lengths is the launches and one event per call.
void device_sends_changed(PatchHandle& h) { h.console.sends.tab_dirty = true; }

void device_sends_drop(PatchHandle& h)
{
    Sends& S = h.console.sends;
    stage_drop(S, {&S.d_tab, &S.d_scratch});
}

int device_buses_send(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_out, void* stream)
{
    Sends& S = h.console.sends;
    int rc;
    if ((rc = S.sync.begin(stream)) != SRACK_OK) return rc;
    if ((rc = S.d_scratch.grow(S.sync, sizeof(float) * S.scratch_rows * 2 * n_samples, "buses_send", "the run sums")) != SRACK_OK) return rc;
    // the tables side by side, each from a 16-byte boundary
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t at_src = 0, at_gain = up16(at_src + sizeof(uint32_t) * S.term_src.size());
    const size_t at_runs = up16(at_gain + sizeof(float) * S.term_gain.size()), at_multi = up16(at_runs + sizeof(uint32_t) * S.runs.size());
    const size_t bytes = up16(at_multi + sizeof(uint32_t) * S.multi.size()) + 16;
    if (S.tab_dirty || !S.d_tab.p) {
        if ((rc = S.d_tab.grow(S.sync, bytes, "buses_send", "the send tables")) != SRACK_OK) return rc;
        S.sync.wait();
        char* tab = (char*)S.d_tab.p;
        HIP_TRY(hipMemcpy(tab + at_src, S.term_src.data(), sizeof(uint32_t) * S.term_src.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(tab + at_gain, S.term_gain.data(), sizeof(float) * S.term_gain.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(tab + at_runs, S.runs.data(), sizeof(uint32_t) * S.runs.size(), hipMemcpyHostToDevice));
        if (!S.multi.empty()) HIP_TRY(hipMemcpy(tab + at_multi, S.multi.data(), sizeof(uint32_t) * S.multi.size(), hipMemcpyHostToDevice));
        S.tab_dirty = false;
    }
    const char* tab = (const char*)S.d_tab.p;
    SendArgs a;
    a.rows = d_rows;
    a.out = d_out;
    a.scratch = (float*)S.d_scratch.p;
    a.term_src = (const uint32_t*)(tab + at_src);
    a.term_gain = (const float*)(tab + at_gain);
    a.runs = (const SendRun*)(tab + at_runs);
    a.multi = (const SendMulti*)(tab + at_multi);
    a.n = n_samples;
    a.row_channels = row_channels;
    a.used = row_channels < 2 ? row_channels : 2u;
    a.n_runs = (uint32_t)(S.runs.size() / 4);
    a.n_multi = (uint32_t)(S.multi.size() / 4);
    a.max_blocks = S.max_blocks;
    launch_sends(a, (hipStream_t)stream);
    if ((rc = S.sync.end(stream)) != SRACK_OK) return rc;
    S.last_sends = (uint32_t)S.src.size();
    S.last_runs = a.n_runs;
    S.ran = true;
    return SRACK_OK;
}

static std::string sends_note(const Sends& S)
{
    return S.ran ? " sends=" + std::to_string(S.last_sends) + "[" + std::to_string(S.last_runs) + " runs]" : std::string();
}

// ---- the bus filters (busvcf.hip.h, launched through launch_bus_filter) -----------------------------------------------------------------
// One lane per (enabled bus, used channel) row.  The row table — where each row lies, its state slot, its bus's sliders and port, and
// the rows of the disabled buses, which an out-of-place call copies — is made again after a change of the setting or of row_channels,
// behind a host-side wait for the last call's kernels, which may still be reading it.  The state is one allocation, zeroed on the
// call's stream when it is fresh; after a change of the enabled set it comes up from the host in its new layout (BusVcf::pending).  A
// tick session of unchanged filters is the launch and one event per call.
static uint32_t busvcf_enabled(const std::vector<uint8_t>& en)
{
    uint32_t n = 0;
    for (uint8_t e : en) n += e != 0;
    return n;
}

// The state as it stands, f32 [slots][kBusVcfFields] in the order of F.enabled; `have` false: there is none, every filter is at zero.
static int busvcf_fetch(BusVcf& F, std::vector<float>& out, bool& have)
{
    have = false;
    if (!F.pending.empty()) {
        out = F.pending;
        have = true;
        return SRACK_OK;
    }
    if (!F.d_state.p || F.fresh) return SRACK_OK;
    const size_t slots = (size_t)2 * busvcf_enabled(F.enabled);
    if (slots == 0) return SRACK_OK;
    F.sync.wait();
    std::vector<float> raw((slots + 63) / 64 * (kBusVcfFields * 64));
    HIP_TRY(hipMemcpy(raw.data(), F.d_state.p, sizeof(float) * raw.size(), hipMemcpyDeviceToHost));
    out.resize(slots * kBusVcfFields);
    for (size_t sl = 0; sl < slots; sl++)
        for (int f = 0; f < kBusVcfFields; f++) out[sl * kBusVcfFields + f] = raw[(sl >> 6) * (kBusVcfFields * 64) + (size_t)f * 64 + (sl & 63)];
    have = true;
    return SRACK_OK;
}

void device_busvcf_changed(PatchHandle& h) { h.console.busvcf.tab_dirty = true; }

void device_busvcf_reset(PatchHandle& h)
{
    h.console.busvcf.pending.clear();
    h.console.busvcf.fresh = true;  // zeroed on the next call's stream, before its kernel
}

int device_busvcf_enable(PatchHandle& h, const std::vector<uint8_t>& enabled)
{
    BusVcf& F = h.console.busvcf;
    if (!F.set || enabled == F.enabled) return SRACK_OK;
    std::vector<float> old;
    bool have = false;
    const int rc = busvcf_fetch(F, old, have);
    if (rc != SRACK_OK) return rc;
    if (!have) return SRACK_OK;  // all zeros, in any layout
    std::vector<float> now((size_t)2 * busvcf_enabled(enabled) * kBusVcfFields, 0.0f);
    size_t from = 0, to = 0;
    for (size_t b = 0; b < enabled.size(); b++) {  // a bus that stays enabled keeps its state; one enabled now starts from zeros; a disabled one drops it
        if (F.enabled[b] && enabled[b]) std::copy(old.begin() + from, old.begin() + from + 2 * kBusVcfFields, now.begin() + to);
        if (F.enabled[b]) from += 2 * kBusVcfFields;
        if (enabled[b]) to += 2 * kBusVcfFields;
    }
    F.pending = std::move(now);
    if (F.pending.empty()) F.fresh = true;
    return SRACK_OK;
}

int device_busvcf_state(PatchHandle& h, float* state, uint32_t cap)
{
    BusVcf& F = h.console.busvcf;
    const size_t n = std::min<size_t>(cap, h.n_buses);
    std::vector<float> cur;
    bool have = false;
    const int rc = busvcf_fetch(F, cur, have);
    if (rc != SRACK_OK) return rc;
    std::fill(state, state + n * 2 * kBusVcfFields, 0.0f);
    size_t from = 0;
    for (size_t b = 0; have && b < n; b++) {
        if (!F.enabled[b]) continue;
        std::copy(cur.begin() + from, cur.begin() + from + 2 * kBusVcfFields, state + b * 2 * kBusVcfFields);
        from += 2 * kBusVcfFields;
    }
    return SRACK_OK;
}

int device_buses_filter(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream)
{
    BusVcf& F = h.console.busvcf;
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t n_buses = h.n_buses, used = row_channels < 2 ? row_channels : 2u;
    const uint32_t n_enabled = busvcf_enabled(F.enabled);
    int rc;
    if ((rc = F.sync.begin(stream)) != SRACK_OK) return rc;
    // the state: two slots per enabled bus, whole waves of 64
    const size_t need = ((size_t)2 * n_enabled + 63) / 64 * 64;
    const size_t state_bytes = sizeof(float) * kBusVcfFields * need;
    if (F.d_state.bytes < state_bytes) {  // (a failure leaves the earlier state, which then is `pending` or nothing)
        if ((rc = F.d_state.grow(F.sync, state_bytes, "buses_filter", "the filters' state")) != SRACK_OK) return rc;
        if (F.pending.empty()) F.fresh = true;
    }
    if (!F.pending.empty()) {
        std::vector<float> raw((size_t)kBusVcfFields * need, 0.0f);
        const size_t slots = F.pending.size() / kBusVcfFields;
        for (size_t sl = 0; sl < slots; sl++)
            for (int f = 0; f < kBusVcfFields; f++) raw[(sl >> 6) * (kBusVcfFields * 64) + (size_t)f * 64 + (sl & 63)] = F.pending[sl * kBusVcfFields + f];
        F.sync.wait();
        HIP_TRY(hipMemcpy(F.d_state.p, raw.data(), sizeof(float) * raw.size(), hipMemcpyHostToDevice));
        F.pending.clear();
        F.fresh = false;
    } else if (F.fresh && need) {  // InternalMoogFilterState::default(): all zeros
        HIP_TRY(hipMemsetAsync(F.d_state.p, 0, state_bytes, st));
        F.fresh = false;
    }
    if (F.tab_dirty || !F.d_tab.p || F.tab_row_channels != row_channels) {
        std::vector<BusVcfRow> rows;
        std::vector<uint32_t> copy;
        uint32_t k = 0;
        for (uint32_t b = 0; b < n_buses; b++) {
            for (uint32_t c = 0; c < used; c++) {
                if (!F.enabled[b]) {
                    copy.push_back(b * row_channels + c);
                    continue;
                }
                BusVcfRow r;
                r.row = b * row_channels + c;
                r.bus = b;
                r.slot = 2 * k + c;
                r.port = (uint32_t)F.port[b];
                r.freq = F.params[(size_t)b * SRACK_BUS_FILTER_NPARAMS + SRACK_VCF_FREQ];
                r.res = F.params[(size_t)b * SRACK_BUS_FILTER_NPARAMS + SRACK_VCF_RES];
                r.exp_amt = F.params[(size_t)b * SRACK_BUS_FILTER_NPARAMS + SRACK_VCF_EXP_AMT];
                r.pad = 0;
                rows.push_back(r);
            }
            k += F.enabled[b] != 0;
        }
        const size_t at_copy = sizeof(BusVcfRow) * rows.size(), bytes = at_copy + sizeof(uint32_t) * copy.size() + 16;
        if ((rc = F.d_tab.grow(F.sync, bytes, "buses_filter", "the table of the rows")) != SRACK_OK) return rc;
        F.sync.wait();
        if (!rows.empty()) HIP_TRY(hipMemcpy(F.d_tab.p, rows.data(), at_copy, hipMemcpyHostToDevice));
        if (!copy.empty()) HIP_TRY(hipMemcpy((char*)F.d_tab.p + at_copy, copy.data(), sizeof(uint32_t) * copy.size(), hipMemcpyHostToDevice));
        F.n_rows = (uint32_t)rows.size();
        F.n_copy = (uint32_t)copy.size();
        F.tab_row_channels = row_channels;
        F.tab_dirty = false;
    }
    BusVcfArgs a;
    a.rows = d_rows;
    a.cv = d_cv;
    a.out = d_out;
    a.state = (float*)F.d_state.p;
    a.tab = (const BusVcfRow*)F.d_tab.p;
    a.copy_rows = (const uint32_t*)((const char*)F.d_tab.p + sizeof(BusVcfRow) * F.n_rows);
    a.n = n_samples;
    a.n_rows = F.n_rows;
    a.n_copy = F.n_copy;
    a.used = used;
    launch_bus_filter(a, st);
    if ((rc = F.sync.end(stream)) != SRACK_OK) return rc;
    F.last_enabled = n_enabled;
    F.last_waves = (F.n_rows + 63) / 64;
    F.ran = true;
    return SRACK_OK;
}

static std::string busvcf_note(const BusVcf& F)
{
    return F.ran ? " busvcf=" + std::to_string(F.last_enabled) + "[" + std::to_string(F.last_waves) + " waves]" : std::string();
}

// ---- the bus VCAs (busvca.hip.h, launched through launch_bus_vca) -------------------------------------------------------------------------
// A table entry and six state values per bus, in bus order: nothing is compacted, so a change of modes moves nothing.  The table goes
// up again after a change of the setting, the state after a change of the set of GATE buses or a reset — both behind a host-side wait
// for the last call's kernel, which may still be using them.  A tick session of unchanged VCAs is the launch and one event per call.

// ADSRModule::new's state: phase 0, mode None, r_val 0, from_a_val 0, the rate, TransitionDetector.last true
static BusState<float, kBusVcaFields>::Fresh busvca_fresh(const BusVca& F)
{
    return {0.0f, (float)SRACK_ADSR_MODE_NONE, 0.0f, 0.0f, F.rate, 1.0f};
}

void device_busvca_changed(PatchHandle& h) { h.console.busvca.tab_dirty = true; }

void device_busvca_reset(PatchHandle& h) { h.console.busvca.state.reset(); }

int device_busvca_modes(PatchHandle& h, const std::vector<int32_t>& mode)
{
    BusVca& F = h.console.busvca;
    if (!F.set) return SRACK_OK;
    return F.state.refresh(F.sync, busvca_fresh(F), h.n_buses, [&](size_t b) { return F.mode[b] == SRACK_BUS_VCA_GATE; }, [&](size_t b) { return mode[b] == SRACK_BUS_VCA_GATE; });
}

int device_busvca_state(PatchHandle& h, float* state, uint32_t cap)
{
    BusVca& F = h.console.busvca;
    return F.state.hand_out(F.sync, busvca_fresh(F), h.n_buses, [&](size_t b) { return F.mode[b] == SRACK_BUS_VCA_GATE; }, state, cap);
}

int device_buses_vca(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_ctl, float* d_out, float* d_env, void* stream)
{
    BusVca& F = h.console.busvca;
    const uint32_t n_buses = h.n_buses;
    int rc;
    if ((rc = F.sync.begin(stream)) != SRACK_OK) return rc;
    const size_t tab_bytes = sizeof(BusVcaBus) * n_buses;
    if (!F.state.d_state.p || !F.d_tab.p) {  // (n_buses is fixed while the VCAs live: another n_buses drops them)
        if ((rc = F.state.alloc(F.sync, n_buses, "buses_vca", "the VCAs' state")) != SRACK_OK) return rc;
        if ((rc = F.d_tab.grow(F.sync, tab_bytes, "buses_vca", "the VCAs' table")) != SRACK_OK) return rc;
        F.tab_dirty = true;
    }
    if ((rc = F.state.upload(F.sync, busvca_fresh(F), n_buses)) != SRACK_OK) return rc;
    uint32_t n_on = 0, n_gated = 0;
    for (uint32_t b = 0; b < n_buses; b++) {
        n_on += F.mode[b] != SRACK_BUS_VCA_OFF;
        n_gated += F.mode[b] == SRACK_BUS_VCA_GATE;
    }
    if (F.tab_dirty) {
        std::vector<BusVcaBus> tab(n_buses);
        for (uint32_t b = 0; b < n_buses; b++) {
            BusVcaBus& r = tab[b];
            r.a_sec = F.params[(size_t)b * SRACK_BUS_VCA_NPARAMS + SRACK_ADSR_A_SEC];
            r.d_sec = F.params[(size_t)b * SRACK_BUS_VCA_NPARAMS + SRACK_ADSR_D_SEC];
            r.s_val = F.params[(size_t)b * SRACK_BUS_VCA_NPARAMS + SRACK_ADSR_S_VAL];
            r.r_sec = F.params[(size_t)b * SRACK_BUS_VCA_NPARAMS + SRACK_ADSR_R_SEC];
            r.mode = (uint32_t)F.mode[b];
            r.negative = F.negative[b];
            r.pad[0] = r.pad[1] = 0;
        }
        F.sync.wait();
        HIP_TRY(hipMemcpy(F.d_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice));
        F.tab_dirty = false;
    }
    BusVcaArgs a;
    a.rows = d_rows;
    a.ctl = d_ctl;
    a.out = d_out;
    a.env = d_env;
    a.state = (float*)F.state.d_state.p;
    a.tab = (const BusVcaBus*)F.d_tab.p;
    a.rate = F.rate;
    a.n = n_samples;
    a.n_buses = n_buses;
    a.row_channels = row_channels;
    a.used = row_channels < 2 ? row_channels : 2u;
    launch_bus_vca(a, (hipStream_t)stream);
    if ((rc = F.sync.end(stream)) != SRACK_OK) return rc;
    F.last_on = n_on;
    F.last_gated = n_gated;
    F.ran = true;
    return SRACK_OK;
}

static std::string busvca_note(const BusVca& F)
{
    return F.ran ? " busvca=" + std::to_string(F.last_on) + "[" + std::to_string(F.last_gated) + " gated]" : std::string();
}

// ---- the bus shapers (busshape.hip.h, launched through launch_bus_shaper) -----------------------------------------------------------------
// A table entry per bus, in bus order, and behind it the list of the buses that are not OFF: an in-place call launches work for those
// alone, an out-of-place one for every bus (an OFF bus is a copy).  There is no state.  The table goes up again after a change of the
// setting, behind a host-side wait for the last call's kernel, which may still be reading it.  A tick session of unchanged shapers is
// the launch and one event per call.
void device_busshaper_changed(PatchHandle& h) { h.console.busshaper.tab_dirty = true; }

int device_buses_shaper(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream)
{
    BusShaper& F = h.console.busshaper;
    const uint32_t n_buses = h.n_buses;
    int rc;
    if ((rc = F.sync.begin(stream)) != SRACK_OK) return rc;
    std::vector<uint32_t> on;
    uint32_t n_cv = 0;
    for (uint32_t b = 0; b < n_buses; b++) {
        if (F.mode[b] != SRACK_BUS_SHAPER_OFF) on.push_back(b);
        n_cv += F.mode[b] == SRACK_BUS_SHAPER_CV;
    }
    const size_t at_list = sizeof(BusShaperBus) * n_buses;
    if (F.tab_dirty || !F.d_tab.p) {  // (n_buses is fixed while the shapers live: another n_buses drops them)
        std::vector<BusShaperBus> tab(n_buses);
        for (uint32_t b = 0; b < n_buses; b++) {
            BusShaperBus& r = tab[b];
            r.pre = F.params[(size_t)b * SRACK_BUS_SHAPER_NPARAMS + SRACK_BUS_SHAPER_PRE];
            r.exponent = F.params[(size_t)b * SRACK_BUS_SHAPER_NPARAMS + SRACK_BUS_SHAPER_EXPONENT];
            r.post = F.params[(size_t)b * SRACK_BUS_SHAPER_NPARAMS + SRACK_BUS_SHAPER_POST];
            r.mode = (uint32_t)F.mode[b];
        }
        if ((rc = F.d_tab.grow(F.sync, at_list + sizeof(uint32_t) * n_buses, "buses_shaper", "the shapers' table")) != SRACK_OK) return rc;
        F.sync.wait();
        HIP_TRY(hipMemcpy(F.d_tab.p, tab.data(), at_list, hipMemcpyHostToDevice));
        if (!on.empty()) HIP_TRY(hipMemcpy((char*)F.d_tab.p + at_list, on.data(), sizeof(uint32_t) * on.size(), hipMemcpyHostToDevice));
        F.tab_dirty = false;
    }
    const bool in_place = d_out == d_rows;
    BusShaperArgs a;
    a.rows = d_rows;
    a.cv = d_cv;
    a.out = d_out;
    a.tab = (const BusShaperBus*)F.d_tab.p;
    a.list = in_place ? (const uint32_t*)((const char*)F.d_tab.p + at_list) : nullptr;
    a.n = n_samples;
    a.n_work = in_place ? (uint32_t)on.size() : n_buses;
    a.n_stretches = (n_samples + kBusShaperStretch - 1) / kBusShaperStretch;
    a.n_units = a.n_work * a.n_stretches;  // (rows of 4 n_units KiB at the least: far below 2^32 in any memory)
    a.row_channels = row_channels;
    a.used = row_channels < 2 ? row_channels : 2u;
    launch_bus_shaper(a, (hipStream_t)stream);
    if ((rc = F.sync.end(stream)) != SRACK_OK) return rc;
    F.last_on = (uint32_t)on.size();
    F.last_cv = n_cv;
    F.ran = true;
    return SRACK_OK;
}

static std::string busshaper_note(const BusShaper& F)
{
    return F.ran ? " busshp=" + std::to_string(F.last_on) + "[" + std::to_string(F.last_cv) + " cv]" : std::string();
}

// ---- the bus meters (busmeter.hip.h, launched through launch_bus_meter) ------------------------------------------------------------------
// A tap: the kernel reads the caller's rows and continues the caller's records.  The stage has no memory of its own, so there is nothing
// to order between its calls beyond what the caller's streams order: a call is the launch and its error.
int device_buses_meter(PatchHandle& h, uint64_t first_sample, uint32_t n_samples, const float* d_rows, uint32_t row_channels, uint32_t window,
                       double* d_levels, uint32_t n_windows, double* d_totals, void* stream)
{
    BusMeter& F = h.console.busmeter;
    (void)n_windows;  // (capi.cpp has held the call's span against it: the kernel's window index stays below it)
    BusMeterArgs a;
    a.rows = d_rows;
    a.levels = d_levels;
    a.totals = d_totals;
    a.first = d_levels ? first_sample : 0;
    a.window = d_levels ? window : 0;
    a.n = n_samples;
    a.n_buses = h.n_buses;
    a.row_channels = row_channels;
    a.used = row_channels < 2 ? row_channels : 2u;
    launch_bus_meter(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    F.last_buses = h.n_buses;
    F.last_window = a.window;
    F.ran = true;
    return SRACK_OK;
}

static std::string busmeter_note(const BusMeter& F)
{
    return F.ran ? " meter=" + std::to_string(F.last_buses) + "[w" + (F.last_window ? std::to_string(F.last_window) : std::string("-")) + "]" : std::string();
}

// ---- the bus oscillators (busosc.hip.h, launched through launch_bus_osc) ---------------------------------------------------------------
// Two state values per bus, in bus order: nothing is compacted, so a change of the enabled set moves nothing.  The table has an entry per
// enabled bus, ordered by (port, antialiasing) so that a wave's lanes share a class wherever they can, and the list of the disabled
// buses behind it.  The table goes up again after a change of the setting, the state after a change of the enabled set or a reset —
// both behind a host-side wait for the last call's kernel, which may still be using them.  A tick session of unchanged oscillators is
// the launch and one event per call.

// OscillatorModule::new's state: pos 0.0, TransitionDetector.last true
static const BusState<double, kBusOscFields>::Fresh kBusOscFresh = {0.0, 1.0};

void device_busosc_changed(PatchHandle& h) { h.console.busosc.tab_dirty = true; }

void device_busosc_reset(PatchHandle& h, const double* pos)
{
    BusOsc& F = h.console.busosc;
    F.state.reset();
    if (!pos) return;
    const size_t n = h.n_buses;
    F.state.pending = F.state.filled(kBusOscFresh, n);
    for (size_t b = 0; b < n; b++)
        if (F.enabled[b]) F.state.pending[b] = pos[b];  // (a disabled bus holds the fresh state)
    F.state.fresh = false;
}

int device_busosc_enable(PatchHandle& h, const std::vector<uint8_t>& enabled)
{
    BusOsc& F = h.console.busosc;
    if (!F.set) return SRACK_OK;
    return F.state.refresh(F.sync, kBusOscFresh, h.n_buses, [&](size_t b) { return F.enabled[b] != 0; }, [&](size_t b) { return enabled[b] != 0; });
}

int device_busosc_state(PatchHandle& h, double* state, uint32_t cap)
{
    BusOsc& F = h.console.busosc;
    return F.state.hand_out(F.sync, kBusOscFresh, h.n_buses, [&](size_t b) { return F.enabled[b] != 0; }, state, cap);
}

int device_buses_osc(PatchHandle& h, uint32_t n_samples, const float* d_cv, const float* d_sync, float* d_out, void* stream)
{
    BusOsc& F = h.console.busosc;
    const uint32_t n_buses = h.n_buses;
    int rc;
    if ((rc = F.sync.begin(stream)) != SRACK_OK) return rc;
    const size_t tab_bytes = sizeof(BusOscBus) * n_buses + sizeof(uint32_t) * n_buses;  // (n_on + n_off = n_buses, and an entry is the larger)
    if (!F.state.d_state.p || !F.d_tab.p) {  // (n_buses is fixed while the oscillators live: another n_buses drops them)
        if ((rc = F.state.alloc(F.sync, n_buses, "buses_osc", "the oscillators' state")) != SRACK_OK) return rc;
        if ((rc = F.d_tab.grow(F.sync, tab_bytes, "buses_osc", "the oscillators' table")) != SRACK_OK) return rc;
        F.tab_dirty = true;
    }
    if ((rc = F.state.upload(F.sync, kBusOscFresh, n_buses)) != SRACK_OK) return rc;
    if (F.tab_dirty) {
        std::vector<BusOscBus> tab;
        std::vector<uint32_t> off;
        tab.reserve(n_buses);
        for (int cls = 0; cls < 6; cls++)  // (port, antialiasing), each class in bus order
            for (uint32_t b = 0; b < n_buses; b++) {
                if (!F.enabled[b] || F.port[b] * 2 + (F.aa[b] ? 1 : 0) != cls) continue;
                const float val = F.params[(size_t)b * SRACK_BUS_OSC_NPARAMS + SRACK_BUS_OSC_VAL];
                BusOscBus r;
                r.delta = 440.0 * std::pow(2.0, (double)val) / F.rate;  // get_freq_in_hz(None) / f64(sample_rate), oscillator.rs:46,132
                r.val = (double)val;
                r.depth = F.params[(size_t)b * SRACK_BUS_OSC_NPARAMS + SRACK_BUS_OSC_DEPTH];
                r.offset = F.params[(size_t)b * SRACK_BUS_OSC_NPARAMS + SRACK_BUS_OSC_OFFSET];
                r.bus = b;
                r.flags = (F.port[b] == SRACK_OSC_OUT_SINE ? OSC_OUT_SINE : F.port[b] == SRACK_OSC_OUT_SQUARE ? OSC_OUT_SQUARE : OSC_OUT_SAW) | (F.aa[b] ? OSC_AA : 0u);
                tab.push_back(r);
            }
        for (uint32_t b = 0; b < n_buses; b++)
            if (!F.enabled[b]) off.push_back(b);
        F.sync.wait();
        if (!tab.empty()) HIP_TRY(hipMemcpy(F.d_tab.p, tab.data(), sizeof(BusOscBus) * tab.size(), hipMemcpyHostToDevice));
        if (!off.empty()) HIP_TRY(hipMemcpy((char*)F.d_tab.p + sizeof(BusOscBus) * tab.size(), off.data(), sizeof(uint32_t) * off.size(), hipMemcpyHostToDevice));
        F.n_on = (uint32_t)tab.size();
        F.n_off = (uint32_t)off.size();
        F.tab_dirty = false;
    }
    BusOscArgs a;
    a.cv = d_cv;
    a.sync = d_sync;
    a.out = d_out;
    a.state = (double*)F.state.d_state.p;
    a.tab = (const BusOscBus*)F.d_tab.p;
    a.off = (const uint32_t*)((const char*)F.d_tab.p + sizeof(BusOscBus) * F.n_on);
    a.sr = F.rate;
    a.n = n_samples;
    a.n_buses = n_buses;
    a.n_on = F.n_on;
    a.n_off = F.n_off;
    launch_bus_osc(a, (hipStream_t)stream);
    if ((rc = F.sync.end(stream)) != SRACK_OK) return rc;
    F.last_on = F.n_on;
    F.last_cv = d_cv != nullptr;
    F.last_sync = d_sync != nullptr;
    F.ran = true;
    return SRACK_OK;
}

static std::string busosc_note(const BusOsc& F)
{
    return F.ran ? " busosc=" + std::to_string(F.last_on) + "[" + (F.last_cv ? "cv" : "-") + (F.last_sync ? "sync" : "-") + "]" : std::string();
}

// ---- the eight together -------------------------------------------------------------------------------------------------------------
void device_console_drop(PatchHandle& h)
{
    Console& C = h.console;
    stage_drop(C.busosc, {&C.busosc.state.d_state, &C.busosc.d_tab});
    busfx_drop(C.busfx);
    stage_drop(C.master, {&C.master.d_gain, &C.master.d_runs});
    device_sends_drop(h);
    stage_drop(C.busvcf, {&C.busvcf.d_state, &C.busvcf.d_tab});
    stage_drop(C.busvca, {&C.busvca.state.d_state, &C.busvca.d_tab});
    stage_drop(C.busshaper, {&C.busshaper.d_tab});
    C.busmeter = BusMeter();
}

std::string device_console_note(const PatchHandle& h)
{
    const Console& C = h.console;
    return sends_note(C.sends) + busosc_note(C.busosc) + busvcf_note(C.busvcf) + busvca_note(C.busvca) + busshaper_note(C.busshaper) + busfx_note(C.busfx) + master_note(C.master) + busmeter_note(C.busmeter);
}

}  // namespace srack
