// series.hip — the series driver: heat_batch_march_series* and heat_batch_set_ambient of the C ABI declared in
// include/heat_amd.h. A series is checked on the host (plan.hpp), its terms are staged on the device, and every step
// calls the march engine (batch.hip) once — through the functions batch.hpp declares and the public C ABI
// (heat_batch_synchronize reports a numerical failure), nothing else; batch.hpp lists the fields of the batch it may touch.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.hpp"
#include "plan.hpp"
#include "series_kernels.hpp"

namespace {

// The per-call device buffers of a series go only when the batch's stream has run dry (declared after them: destroyed first).
struct SeriesDrain {
    heat_batch *b;
    ~SeriesDrain() { (void)hipStreamSynchronize(b->stream); }
};
#define SERIES_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

template <typename T>
int series_alloc(DevBuf<T> &buf, size_t count, const char *what, const T *src = nullptr) {
    hipError_t e = buf.alloc(count);
    if (e == hipSuccess && count > 0 && src) e = hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail(HEAT_E_DEVICE, "series march: %s (%zu bytes) on the device: %s — nothing has been marched", what, count * sizeof(T),
                    hipGetErrorString(e));
    return HEAT_OK;
}
template <typename T>
int series_upload(DevBuf<T> &buf, const T *src, size_t count, const char *what) { return series_alloc(buf, count, what, src); }
template <typename T>
int series_upload(DevBuf<T> &buf, const std::vector<T> &src, const char *what) { return series_alloc(buf, src.size(), what, src.data()); }
// An in/out array of a call: absent (nullptr: no device copy), uploaded (resume), or allocated for the device to initialise.
template <typename T>
int report_array(DevBuf<T> &buf, const T *host, size_t count, bool upload, const char *what) {
    return host ? series_alloc(buf, count, what, upload ? host : nullptr) : HEAT_OK;
}
// Back to the host behind the stream's work (and the copy that gave e, if that went well); nothing where either side holds no copy.
template <typename T>
hipError_t series_fetch(T *host, const DevBuf<T> &buf, hipStream_t st, hipError_t e = hipSuccess) {
    return e != hipSuccess || !host || !buf.p ? e : hipMemcpyAsync(host, buf.p, buf.n * sizeof(T), hipMemcpyDeviceToHost, st);
}
// Row k of a buffer of rows of n values; nullptr where the buffer is absent.
template <typename T>
T *row(const DevBuf<T> &buf, int k, int64_t n) { return buf.p ? buf.p + (size_t)k * (size_t)n : nullptr; }
// dst[d] = src[orig_of[d]]: an array over the caller's surfaces, in the device's order.
template <typename T>
void to_device_order(heat_batch *b, const T *src, T *dst) {
    const int64_t *orig_of = b->h_orig_of.data();
    b->pool->run(b->n_surf, [&](int64_t d0, int64_t d1) { for (int64_t d = d0; d < d1; d++) dst[d] = src[orig_of[d]]; });
}
// The start of a fresh run's accumulator on the device (the step numbers start at -1, written as 0xff bytes).
inline hipError_t series_fill(const DevBuf<double> &d, double v, hipStream_t st) { launch_fill_f64(d.p, (int64_t)d.n, v, st); return hipSuccess; }
inline hipError_t series_fill(const DevBuf<int64_t> &d, int64_t v, hipStream_t st) {
    return d.p ? hipMemsetAsync(d.p, v < 0 ? 0xff : 0, d.n * sizeof(int64_t), st) : hipSuccess;
}
// An in/out accumulator: the caller's array, its device copy, a fresh run's start value and the device view's field for the copy.
template <typename T>
struct Acc {
    T *host = nullptr, **view = nullptr;
    T init = 0;
    DevBuf<T> dev;
    void bind(T *h, T v, T **field) { host = h, init = v, view = field; }
    // uploaded on resume, else allocated; nothing where the caller passes no array
    int stage(size_t n, bool resume, const char *w) { const int rc = report_array(dev, host, n, resume, w); *view = dev.p; return rc; }
    hipError_t start(hipStream_t st, hipError_t e = hipSuccess) { return e != hipSuccess ? e : series_fill(dev, init, st); }
    hipError_t fetch(hipStream_t st, hipError_t e = hipSuccess) { return series_fetch(host, dev, st, e); }
};
// start() or fetch() of every accumulator of a list, in order, up to the first error
template <typename A, size_t N>
hipError_t for_each_acc(A (&acc)[N], hipError_t (A::*what)(hipStream_t, hipError_t), hipStream_t st, hipError_t e = hipSuccess) {
    for (A &a : acc) e = (a.*what)(st, e);
    return e;
}

// ---- the terms of a series march: each owns its host tables (prepare: no device call), its device buffers and view (upload:
// through the null stream) and its way back (fetch: asynchronous). Declared before the call's SeriesDrain: freed after the stream ran dry. ----

// The driven inputs: channel numbers and gains per DEVICE surface, structure of arrays; the own-face bits and face nodes.
// The gain arrays serve the sky, the solar gains and the room radiation too.
struct InputsTerm {
    const double *gain[4] = {nullptr, nullptr, nullptr, nullptr};
    bool driven = false;
    std::vector<int32_t> h_chan;
    std::vector<double> h_gain[4];
    std::vector<uint8_t> h_own;
    std::vector<uint32_t> h_face;
    DevBuf<int32_t> chan;
    DevBuf<double> d_gain[4];
    DevBuf<uint8_t> own;
    DevBuf<uint32_t> face;
    SeriesInputs view{};
    // gain[a] in device order, once: for whichever term drives input a first
    void need_gain(heat_batch *b, int a) {
        if (!gain[a] || !h_gain[a].empty()) return;
        h_gain[a].resize((size_t)b->n_surf);
        to_device_order(b, gain[a], h_gain[a].data());
    }
    void prepare(heat_batch *b, const heat_series *s) {
        const int64_t S = b->n_surf;
        const int32_t *src[4] = {s->solar_front_chan, s->solar_back_chan, s->ir_front_chan, s->ir_back_chan};
        const double *g[4] = {s->solar_front_gain, s->solar_back_gain, s->ir_front_gain, s->ir_back_gain};
        bool own_any = false;
        for (int a = 0; a < 4; a++) {
            gain[a] = g[a];
            for (int64_t q = 0; src[a] && q < S && !driven; q++) driven = src[a][q] >= 0;
        }
        for (int64_t q = 0; s->ir_own_face && q < S && !own_any; q++) own_any = (s->ir_own_face[q] & 3) != 0;
        if (!driven) return;
        h_chan.assign(4 * (size_t)S, -1);
        for (int a = 0; a < 4; a++) {
            if (!src[a]) continue;
            to_device_order(b, src[a], h_chan.data() + (size_t)a * S);
            need_gain(b, a);
        }
        if (!own_any) return;
        const int64_t *orig_of = b->h_orig_of.data();
        h_own.resize((size_t)S);
        h_face.resize(2 * (size_t)S);
        b->pool->run(S, [&](int64_t d0, int64_t d1) {
            for (int64_t d = d0; d < d1; d++) {
                const int64_t q = orig_of[d];
                h_own[d] = (uint8_t)(s->ir_own_face[q] & 3);
                h_face[d] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], 0);
                h_face[S + d] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], (int)b->h_node_count[q] - 1);
            }
        });
    }
    int upload() {
        SERIES_TRY(series_upload(chan, h_chan, "channel numbers"));
        for (int a = 0; a < 4; a++) SERIES_TRY(series_upload(d_gain[a], h_gain[a], "gains"));
        SERIES_TRY(series_upload(own, h_own, "own-face bits"));
        SERIES_TRY(series_upload(face, h_face, "face node table"));
        view.chan = chan.p, view.own_face = own.p, view.face = face.p;
        for (int a = 0; a < 4; a++) view.gain[a] = d_gain[a].p;
        return HEAT_OK;
    }
};

// The probes: (buffer, index) of every probed slot; the trace; the record of the first failed step.
struct ProbesTerm {
    int64_t P = 0;
    std::vector<uint8_t> h_buf;
    std::vector<uint32_t> h_idx;
    DevBuf<uint8_t> buf;
    DevBuf<uint32_t> idx;
    DevBuf<int> failed;  // the step, then the flags as they were after it
    DevBuf<double> trace;
    static void place(const heat_batch *b, int kind, int64_t index, int node, uint8_t &buf, uint32_t &idx) {
        if (kind == PROBE_ZONE) {
            buf = (uint8_t)kProbeBufZone, idx = (uint32_t)index;
        } else if (kind == PROBE_NODE) {
            buf = (uint8_t)kProbeBufT, idx = (uint32_t)node_slot_index(b->h_node_tile_base[index], b->h_node_geom[index], node);
        } else {  // hs front, hs back, flow front, flow back: SideOut record side * S + d, as doubles
            const int a = kind - PROBE_HS_FRONT;
            const int64_t rec = (int64_t)(a & 1) * b->n_surf + b->h_dev_of[index];
            buf = (uint8_t)kProbeBufOut, idx = (uint32_t)(2 * rec + (a >> 1));
        }
    }
    int prepare(heat_batch *b, const heat_series *s) {
        P = s->n_probes;
        h_buf.resize((size_t)P);
        h_idx.resize((size_t)P);
        for (int64_t p = 0; p < P; p++) {
            int kind = 0, node = 0;
            int64_t index = 0;
            if (!b->resolver->resolve(s->probe_slot[p], kind, index, node)) return fail(HEAT_E_SIZE, "probe %lld: slot not resolved", (long long)p);
            place(b, kind, index, node, h_buf[p], h_idx[p]);
        }
        return HEAT_OK;
    }
    int upload(const double *host_trace, int n_steps) {
        const int fail_init[5] = {-1, 0, 0, 0, 0};
        SERIES_TRY(series_upload(buf, h_buf, "probe table"));
        SERIES_TRY(series_upload(idx, h_idx, "probe table"));
        SERIES_TRY(series_upload(failed, fail_init, 5, "failed step"));
        return host_trace ? series_alloc(trace, (size_t)n_steps * P, "trace") : HEAT_OK;
    }
    hipError_t fetch(double *host_trace, hipStream_t st) { return series_fetch(host_trace, trace, st); }
};

// The zone loads: the term lists sorted by zone with CSR offsets (plan.hpp), the mode bytes in the caller's order, the applied rows.
struct LoadsTerm {
    bool on = false;
    int64_t NT = 0;
    ZoneLoadTables zt;
    std::vector<uint8_t> h_mode;
    DevBuf<int32_t> i32;
    DevBuf<double> f64, applied;
    DevBuf<uint8_t> mode;
    ZoneLoadsDev view{};
    void prepare(const heat_batch *b, const heat_zone_loads *l) {
        on = l && (l->n_gains > 0 || l->n_flows > 0 || l->n_thermostats > 0);
        if (!on) return;
        NT = l->n_thermostats;
        build_zone_load_tables(b->n_zones, l, zt);
        h_mode.assign((size_t)NT, 0);
        if (l->th_mode) std::copy(l->th_mode, l->th_mode + NT, h_mode.begin());
    }
    int upload(const double *host_applied, int n_steps) {
        if (!on) return HEAT_OK;
        // (packed into two uploads, not thirteen: each one is an allocation and a pageable copy in the call's set-up)
        const std::vector<int32_t> *a_i32[8] = {&zt.off, &zt.gain_chan, &zt.flow_volume_chan, &zt.flow_temp_chan, &zt.th_sensor,
                                                &zt.th_heat_chan, &zt.th_cool_chan, &zt.th_orig};
        const std::vector<double> *a_f64[5] = {&zt.gain_factor, &zt.flow_volume_gain, &zt.th_heat_power, &zt.th_cool_power, &zt.th_half_band};
        const int32_t **v_i32[8] = {&view.off, &view.gain_chan, &view.flow_volume_chan, &view.flow_temp_chan, &view.th_sensor,
                                    &view.th_heat_chan, &view.th_cool_chan, &view.th_orig};
        const double **v_f64[5] = {&view.gain_factor, &view.flow_volume_gain, &view.th_heat_power, &view.th_cool_power, &view.th_half_band};
        std::vector<int32_t> h_i32;
        std::vector<double> h_f64;
        for (auto *v : a_i32) h_i32.insert(h_i32.end(), v->begin(), v->end());
        for (auto *v : a_f64) h_f64.insert(h_f64.end(), v->begin(), v->end());
        SERIES_TRY(series_upload(i32, h_i32, "zone load tables"));
        SERIES_TRY(series_upload(f64, h_f64, "zone load tables"));
        SERIES_TRY(series_upload(mode, h_mode, "thermostat modes"));
        if (host_applied) SERIES_TRY(series_alloc(applied, (size_t)n_steps * NT, "applied powers"));
        for (size_t a = 0, at = 0; a < 8; at += a_i32[a++]->size()) *v_i32[a] = i32.p + at;
        for (size_t a = 0, at = 0; a < 5; at += a_f64[a++]->size()) *v_f64[a] = f64.p + at;
        view.th_mode = mode.p;
        return HEAT_OK;
    }
    hipError_t fetch(const heat_zone_loads *l, double *host_applied, hipStream_t st) {
        return on ? series_fetch(l->th_mode, mode, st, series_fetch(host_applied, applied, st)) : hipSuccess;
    }
};

// The report (heat_series_report): the group entries sorted into device order (buffer, index) and cut into segments
// (plan.hpp), the step's group sums, the group trace, the limits (always uploaded, never fetched), the accumulators.
struct ReportTerm {
    heat_series_report *r = nullptr;
    int64_t G = 0, Q = 0;
    bool th_stats = false, q_stats = false;
    GroupTables gt;
    std::vector<uint8_t> h_gbuf;
    std::vector<uint32_t> h_gidx;
    DevBuf<uint8_t> gbuf, prev;
    DevBuf<uint32_t> gidx, seg, part_off;
    DevBuf<double> gw, part, group_trace, applied_row, lo, hi;
    Acc<double> q_f64[5], th_f64[2];   // q_min, q_max, q_sum, q_deg_below, q_deg_above; th_sum_heating, th_sum_cooling
    Acc<int64_t> q_i64[4], th_i64[3];  // q_step_min, q_step_max, q_n_below, q_n_above; th_steps_heating, th_steps_cooling, th_switches
    SeriesGroupsDev groups{};
    SeriesStatsDev stats{};
    SeriesThStatsDev th{};
    void prepare(const heat_batch *b, heat_series_report *r_, int64_t P, const std::vector<ResolvedSlot> &entry) {
        r = r_;
        Q = P;
        if (!r) return;
        const double inf = std::numeric_limits<double>::infinity();
        q_f64[0].bind(r->q_min, inf, &stats.q_min), q_f64[1].bind(r->q_max, -inf, &stats.q_max), q_f64[2].bind(r->q_sum, 0.0, &stats.q_sum);
        q_f64[3].bind(r->q_deg_below, 0.0, &stats.q_deg_below), q_f64[4].bind(r->q_deg_above, 0.0, &stats.q_deg_above);
        q_i64[0].bind(r->q_step_min, -1, &stats.q_step_min), q_i64[1].bind(r->q_step_max, -1, &stats.q_step_max);
        q_i64[2].bind(r->q_n_below, 0, &stats.q_n_below), q_i64[3].bind(r->q_n_above, 0, &stats.q_n_above);
        th_f64[0].bind(r->th_sum_heating, 0.0, &th.sum_heating), th_f64[1].bind(r->th_sum_cooling, 0.0, &th.sum_cooling);
        th_i64[0].bind(r->th_steps_heating, 0, &th.steps_heating), th_i64[1].bind(r->th_steps_cooling, 0, &th.steps_cooling);
        th_i64[2].bind(r->th_switches, 0, &th.switches);
        th_stats = th_f64[0].host || th_f64[1].host || th_i64[0].host || th_i64[1].host || th_i64[2].host;
        G = r->n_groups;
        Q = P + G;
        if (G == 0) return;
        const int64_t n_entries = r->group_offset[G];
        std::vector<uint64_t> key((size_t)n_entries);
        for (int64_t i = 0; i < n_entries; i++) {
            uint8_t buf = 0;
            uint32_t idx = 0;
            ProbesTerm::place(b, entry[(size_t)i].kind, entry[(size_t)i].index, entry[(size_t)i].node, buf, idx);
            key[(size_t)i] = (uint64_t)buf << 32 | idx;
        }
        build_group_tables(G, r->group_offset, r->group_weight, key.data(), gt);
        h_gbuf.resize((size_t)n_entries);
        h_gidx.resize((size_t)n_entries);
        for (int64_t i = 0; i < n_entries; i++) h_gbuf[(size_t)i] = (uint8_t)(gt.key[(size_t)i] >> 32), h_gidx[(size_t)i] = (uint32_t)gt.key[(size_t)i];
    }
    int upload(int n_steps, const ProbesTerm &probes, const LoadsTerm &loads) {
        if (!r) return HEAT_OK;
        const bool resume = r->resume != 0;
        const size_t n_wave = gt.wave_seg.size() / 3, n_row = gt.row_seg.size() / 3;
        std::vector<uint32_t> h_seg(gt.wave_seg);
        h_seg.insert(h_seg.end(), gt.row_seg.begin(), gt.row_seg.end());
        SERIES_TRY(series_upload(gbuf, h_gbuf, "group tables"));
        SERIES_TRY(series_upload(gidx, h_gidx, "group tables"));
        SERIES_TRY(series_upload(gw, gt.weight, "group tables"));
        SERIES_TRY(series_upload(seg, h_seg, "group tables"));
        SERIES_TRY(series_upload(part_off, gt.part_off.data(), G > 0 ? gt.part_off.size() : 0, "group tables"));
        SERIES_TRY(series_alloc(part, n_wave + n_row, "group sums"));
        SERIES_TRY(report_array(group_trace, r->group_trace, (size_t)n_steps * G, false, "group trace"));
        for (auto &a : q_f64) SERIES_TRY(a.stage((size_t)Q, resume, "statistics"));
        SERIES_TRY(report_array(lo, r->q_lo, (size_t)Q, true, "statistics"));
        SERIES_TRY(report_array(hi, r->q_hi, (size_t)Q, true, "statistics"));
        for (auto &a : q_i64) SERIES_TRY(a.stage((size_t)Q, resume, "statistics"));
        groups.buf = gbuf.p, groups.idx = gidx.p, groups.weight = gw.p, groups.part = part.p;
        groups.wave_seg = seg.p, groups.row_seg = seg.p + 3 * n_wave, groups.n_wave = (int)n_wave, groups.n_row = (int)n_row;
        stats.n_probes = probes.P, stats.n_groups = G, stats.buf = probes.buf.p, stats.idx = probes.idx.p;
        stats.part = part.p, stats.part_off = part_off.p;
        // (a limit nothing is counted against is not read)
        stats.q_lo = stats.q_n_below || stats.q_deg_below ? lo.p : nullptr;
        stats.q_hi = stats.q_n_above || stats.q_deg_above ? hi.p : nullptr;
        q_stats = Q > 0 && (stats.q_min || stats.q_max || stats.q_sum || stats.q_n_below || stats.q_deg_below || stats.q_n_above ||
                            stats.q_deg_above || group_trace.p);
        if (!th_stats) return HEAT_OK;  // (check_series_report: only with thermostats)
        for (auto &a : th_f64) SERIES_TRY(a.stage((size_t)loads.NT, resume, "thermostat statistics"));
        for (auto &a : th_i64) SERIES_TRY(a.stage((size_t)loads.NT, resume, "thermostat statistics"));
        SERIES_TRY(series_upload(prev, loads.h_mode, "thermostat modes"));
        // (the powers of the step: a row of the applied buffer, or one row of scratch where the caller takes none)
        if (!loads.applied.p && (th_f64[0].host || th_f64[1].host)) SERIES_TRY(series_alloc(applied_row, (size_t)loads.NT, "applied powers"));
        th.prev = prev.p;
        return HEAT_OK;
    }
    // start (a fresh run: min = +inf, max = -inf, steps = -1, sums and counts 0) or fetch of the accumulators
    hipError_t each(hipError_t (Acc<double>::*f64)(hipStream_t, hipError_t), hipError_t (Acc<int64_t>::*i64)(hipStream_t, hipError_t), hipStream_t st,
                    hipError_t e = hipSuccess) {
        return for_each_acc(th_i64, i64, st, for_each_acc(th_f64, f64, st, for_each_acc(q_i64, i64, st, for_each_acc(q_f64, f64, st, e))));
    }
    hipError_t start(hipStream_t st) { return r && r->resume == 0 ? each(&Acc<double>::start, &Acc<int64_t>::start, st) : hipSuccess; }
    hipError_t fetch(hipStream_t st) {
        return r ? each(&Acc<double>::fetch, &Acc<int64_t>::fetch, st, series_fetch(r->group_trace, group_trace, st)) : hipSuccess;
    }
};

// The ideal loads (heat_ideal_loads): tables, the step's setpoints and q-sums, the ideal_q rows, the accumulators.
struct IdealTerm {
    heat_ideal_loads *il = nullptr;
    int64_t NI = 0;
    std::vector<int32_t> h_i32;  // load_of_zone [Z] | heat_chan [N] | cool_chan [N]
    std::vector<double> h_cap;   // heat_cap [N] | cool_cap [N]
    DevBuf<int32_t> i32;
    DevBuf<double> cap, step, q; // step: setpoint [2][N] | qsum [N]; q: ideal_q [n_steps][N]
    Acc<double> f64[4];          // sum_heating, sum_cooling, peak_heating, peak_cooling
    Acc<int64_t> i64[4];         // step_peak_heating, step_peak_cooling, n_sat_heating, n_sat_cooling
    IdealLoadsDev view{};
    void prepare(heat_ideal_loads *il_, const std::vector<int32_t> &load_of_zone) {
        il = il_;
        NI = il ? il->n_loads : 0;
        if (NI == 0) return;
        const double inf = std::numeric_limits<double>::infinity();
        h_i32 = load_of_zone;
        h_i32.insert(h_i32.end(), il->heat_chan, il->heat_chan + NI);
        h_i32.insert(h_i32.end(), il->cool_chan, il->cool_chan + NI);
        h_cap.assign(2 * (size_t)NI, inf);
        if (il->heat_cap) std::copy(il->heat_cap, il->heat_cap + NI, h_cap.begin());
        if (il->cool_cap) std::copy(il->cool_cap, il->cool_cap + NI, h_cap.begin() + NI);
        f64[0].bind(il->sum_heating, 0.0, &view.sum_heating), f64[1].bind(il->sum_cooling, 0.0, &view.sum_cooling);
        f64[2].bind(il->peak_heating, -inf, &view.peak_heating), f64[3].bind(il->peak_cooling, inf, &view.peak_cooling);
        i64[0].bind(il->step_peak_heating, -1, &view.step_peak_heating), i64[1].bind(il->step_peak_cooling, -1, &view.step_peak_cooling);
        i64[2].bind(il->n_sat_heating, 0, &view.n_sat_heating), i64[3].bind(il->n_sat_cooling, 0, &view.n_sat_cooling);
    }
    int upload(const heat_batch *b, const double *host_q, int n_steps) {
        if (NI == 0) return HEAT_OK;
        const bool resume = il->resume != 0;
        SERIES_TRY(series_upload(i32, h_i32, "ideal load tables"));
        SERIES_TRY(series_upload(cap, h_cap, "ideal load tables"));
        SERIES_TRY(series_alloc(step, 3 * (size_t)NI, "ideal load setpoints"));
        if (host_q) SERIES_TRY(series_alloc(q, (size_t)n_steps * NI, "ideal powers"));
        for (auto &a : f64) SERIES_TRY(a.stage((size_t)NI, resume, "ideal load accumulators"));
        for (auto &a : i64) SERIES_TRY(a.stage((size_t)NI, resume, "ideal load accumulators"));
        view.n_loads = (int)NI;
        view.load_of_zone = i32.p, view.heat_chan = i32.p + b->n_zones, view.cool_chan = i32.p + b->n_zones + NI;
        view.heat_cap = cap.p, view.cool_cap = cap.p + NI, view.setpoint = step.p, view.qsum = step.p + 2 * NI;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        return NI > 0 && il->resume == 0 ? for_each_acc(i64, &Acc<int64_t>::start, st, for_each_acc(f64, &Acc<double>::start, st)) : hipSuccess;
    }
    hipError_t fetch(double *host_q, hipStream_t st) {
        return for_each_acc(i64, &Acc<int64_t>::fetch, st, for_each_acc(f64, &Acc<double>::fetch, st, series_fetch(host_q, q, st)));
    }
};

// The sky (heat_sky): the mode bytes and normals per DEVICE surface, the record table as given (the solar gains and the
// shades read it too).
struct SkyTerm {
    unsigned bits = 0;
    std::vector<uint8_t> h_mode;
    std::vector<double> h_normal;
    DevBuf<uint8_t> mode;      // [S]
    DevBuf<double> normal;     // [3][S]
    DevBuf<SkyRecord> record;  // [n_steps][n_sites]
    SeriesSky view{};
    void prepare(heat_batch *b, const heat_sky *sky, InputsTerm &in) {
        if (!bits) return;
        const int64_t S = b->n_surf;
        const int64_t *orig_of = b->h_orig_of.data();
        h_mode.resize((size_t)S);
        h_normal.resize(3 * (size_t)S);
        b->pool->run(S, [&](int64_t d0, int64_t d1) {
            for (int64_t d = d0; d < d1; d++) {
                const int64_t q = orig_of[d];
                const bool on = sky->mode[q] != 0;  // (the normals of the other surfaces are not read, not even here)
                h_mode[d] = sky->mode[q];
                h_normal[d] = on ? sky->normal_x[q] : 0.0;
                h_normal[S + d] = on ? sky->normal_y[q] : 0.0;
                h_normal[2 * S + d] = on ? sky->normal_z[q] : 0.0;
            }
        });
        for (int a = 0; a < 4; a++) if (bits >> a & 1) in.need_gain(b, a);
    }
    // records_read: by the sky's own sides, by apertures or by shades
    int upload(const heat_batch *b, const heat_series *s, const heat_sky *sky, bool records_read, const InputsTerm &in) {
        if (records_read)
            SERIES_TRY(series_upload(record, reinterpret_cast<const SkyRecord *>(sky->record), (size_t)s->n_steps * b->n_sites, "sky records"));
        if (!bits) return HEAT_OK;
        SERIES_TRY(series_upload(mode, h_mode, "sky modes"));
        SERIES_TRY(series_upload(normal, h_normal, "sky normals"));
        view.mode = mode.p, view.normal = normal.p, view.site = b->n_sites > 1 ? b->d_site.p : nullptr;
        for (int a = 0; a < 4; a++) view.gain[a] = in.d_gain[a].p;
        return HEAT_OK;
    }
};
static_assert(sizeof(SkyRecord) == sizeof(heat_sky_record) && sizeof(heat_sky_record) == 64, "SkyRecord mirrors heat_sky_record");

// The shades (heat_shades): the table as structure of arrays (plan.hpp, ShadeTables), every shade's site and horizon, the horizon
// profiles, the step's sunlit fractions, the shade numbers of the sides per DEVICE surface and of the apertures, the sunlit rows.
struct ShadesTerm {
    int64_t NS = 0;
    ShadeTables sht;
    std::vector<int32_t> h_i32, h_side;
    DevBuf<double> tab, tan2, f, sunlit;  // [kShadeRows][NS], [NH][16], [NS], [n_steps][NS]
    DevBuf<double> eff;                   // [3][NS] the effective factors k_series_blinds writes; absent without blinds
    DevBuf<int32_t> i32, side, aperture;  // site [NS] | horizon [NS], [2][S], [NA]
    SeriesShades view{};
    // what a shaded consumer reads: the step's fractions, the diffuse and the ground factors (all NULL without shades) — with
    // blinds (heat_blinds) the effective ones of the step
    ShadeFactors factors() const {
        if (eff.p) return ShadeFactors{eff.p, eff.p + (size_t)NS, eff.p + 2 * (size_t)NS};
        return ShadeFactors{f.p, tab.p + (size_t)SH_FD * NS, tab.p + (size_t)SH_FG * NS};
    }
    void prepare(heat_batch *b, const heat_shades *shades, unsigned sky_bits) {
        NS = shades ? shades->n_shades : 0;  // (a side or aperture needs a shade to refer to: none is shaded without)
        if (NS == 0) return;
        build_shade_tables(shades, sht);
        h_i32.assign(2 * (size_t)NS, 0);
        for (int64_t j = 0; j < NS; j++) {
            h_i32[j] = b->h_site.empty() ? 0 : b->h_site[b->h_dev_of[shades->sh_surface[j]]];
            h_i32[NS + j] = sht.horizon[j];
        }
        if (!(sky_bits & 3) || !(shades->front_shade || shades->back_shade)) return;
        h_side.assign(2 * (size_t)b->n_surf, -1);
        if (shades->front_shade) to_device_order(b, shades->front_shade, h_side.data());
        if (shades->back_shade) to_device_order(b, shades->back_shade, h_side.data() + b->n_surf);
    }
    int upload(const heat_shades *shades, int64_t NA, const double *host_sunlit, int n_steps, bool blinds, SkyTerm &sky) {
        if (NS == 0) return HEAT_OK;
        if (blinds) SERIES_TRY(series_alloc(eff, 3 * (size_t)NS, "effective shade factors"));
        SERIES_TRY(series_upload(tab, sht.f64, "shade table"));
        SERIES_TRY(series_upload(i32, h_i32, "shade table"));
        SERIES_TRY(series_upload(tan2, shades->horizon_tan2, 16 * (size_t)shades->n_horizons, "horizon profiles"));
        SERIES_TRY(series_alloc(f, (size_t)NS, "sunlit fractions"));
        SERIES_TRY(series_upload(side, h_side, "shade numbers"));
        if (NA > 0 && shades->aperture_shade) SERIES_TRY(series_upload(aperture, shades->aperture_shade, (size_t)NA, "shade numbers"));
        if (host_sunlit) SERIES_TRY(series_alloc(sunlit, (size_t)n_steps * NS, "sunlit fractions"));
        view.n = (int)NS, view.site = i32.p, view.horizon = i32.p + NS, view.tab = tab.p, view.tan2 = tan2.p, view.f = f.p;
        sky.view.shade = side.p, sky.view.sf = factors();
        return HEAT_OK;
    }
    hipError_t fetch(double *host_sunlit, hipStream_t st) { return series_fetch(host_sunlit, sunlit, st); }
};

// The blinds (heat_blinds): the blind of every shade and the blinds as structures of arrays (plan.hpp, BlindTables), the state
// bytes, the accumulators (uploaded where the caller passes them), the position and blind_incident rows in the caller's order.
// It reads the shades' site numbers, table and fractions and writes the shades' effective factors: uploaded behind them.
struct BlindsTerm {
    heat_blinds *blinds = nullptr;
    int64_t NL = 0;
    BlindTables blt;
    std::vector<uint8_t> h_state;
    DevBuf<int32_t> of_shade, i32;       // [NS], [kBlindI32Rows][NL]
    DevBuf<double> f64, position, incident;  // [kBlindF64Rows][NL], [n_steps][NL], [n_steps][NL]
    DevBuf<uint8_t> state;               // [NL]
    Acc<double> sum_position;
    Acc<int64_t> steps_closed, switches;
    SeriesBlinds view{};
    void prepare(heat_blinds *blinds_, int64_t NS) {
        blinds = blinds_;
        NL = blinds ? blinds->n_blinds : 0;
        if (NL == 0) return;
        build_blind_tables(NS, blinds, blt);
        h_state.assign((size_t)NL, 0);
        if (blinds->state) std::copy(blinds->state, blinds->state + NL, h_state.begin());
        sum_position.bind(blinds->sum_position, 0.0, &view.sum_position), steps_closed.bind(blinds->steps_closed, 0, &view.steps_closed);
        switches.bind(blinds->switches, 0, &view.switches);
    }
    int upload(const ShadesTerm &shades, const double *host_position, const double *host_incident, int n_steps) {
        if (NL == 0) return HEAT_OK;
        SERIES_TRY(series_upload(of_shade, blt.blind_of_shade, "blind tables"));
        SERIES_TRY(series_upload(i32, blt.i32, "blind tables"));
        SERIES_TRY(series_upload(f64, blt.f64, "blind tables"));
        SERIES_TRY(series_upload(state, h_state, "blind states"));
        SERIES_TRY(sum_position.stage((size_t)NL, true, "blind accumulators"));
        SERIES_TRY(steps_closed.stage((size_t)NL, true, "blind accumulators"));
        SERIES_TRY(switches.stage((size_t)NL, true, "blind accumulators"));
        if (host_position) SERIES_TRY(series_alloc(position, (size_t)n_steps * NL, "blind positions"));
        if (host_incident) SERIES_TRY(series_alloc(incident, (size_t)n_steps * NL, "blind irradiances"));
        view.n_shades = (int)shades.NS, view.n_blinds = (int)NL, view.blind_of_shade = of_shade.p;
        view.site = shades.view.site, view.tab = shades.tab.p, view.f = shades.f.p;
        view.pos_chan = i32.p + BL_POS_CHAN * NL, view.zone = i32.p + BL_ZONE * NL, view.set_chan = i32.p + BL_SET_CHAN * NL;
        view.enable_chan = i32.p + BL_ENABLE_CHAN * NL;
        view.beam_closed = f64.p + BL_BEAM * NL, view.diffuse_closed = f64.p + BL_DIFFUSE * NL, view.ground_closed = f64.p + BL_GROUND * NL;
        view.irr_close = f64.p + BL_IRR_CLOSE * NL, view.irr_open = f64.p + BL_IRR_OPEN * NL, view.half_band = f64.p + BL_HALF_BAND * NL;
        view.state = state.p;
        view.eff_f = shades.eff.p, view.eff_diffuse = shades.eff.p + shades.NS, view.eff_ground = shades.eff.p + 2 * shades.NS;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_position, double *host_incident, hipStream_t st) {
        if (NL == 0) return hipSuccess;
        const hipError_t e = series_fetch(blinds->state, state, st, series_fetch(host_incident, incident, st, series_fetch(host_position, position, st)));
        return switches.fetch(st, steps_closed.fetch(st, sum_position.fetch(st, e)));
    }
};

// The solar gains (heat_solar_gains): the apertures as structure of arrays, the entries as sliced ELL over the receivers in
// device record order (plan.hpp, SolarGainTables), the step's (Pb, Pd), ap_sum (always uploaded) and the transmitted rows.
struct GainsTerm {
    int64_t NA = 0;
    std::vector<int32_t> h_ap_dev;
    std::vector<double> h_ap_f64;
    SolarGainTables gnt;
    DevBuf<int32_t> ap_dev, ap;                 // [NA]; the entries' apertures
    DevBuf<double> ap_f64, transmitted, share;  // normal [3][NA] | coef [6][NA] | tau_diffuse [NA] | scale [NA]; [n_steps][NA]
    DevBuf<double2> power;                      // [NA]
    DevBuf<uint32_t> rec;
    DevBuf<int64_t> slice_off;
    Acc<double> sum;
    SeriesApertures apertures{};
    SeriesGains view{};
    void prepare(heat_batch *b, const heat_solar_gains *gains, InputsTerm &in) {
        NA = gains ? gains->n_apertures : 0;  // (entries need an aperture: there are none without)
        if (NA == 0) return;
        const int64_t S = b->n_surf;
        h_ap_dev.resize((size_t)NA);
        h_ap_f64.resize(11 * (size_t)NA);
        for (int64_t a = 0; a < NA; a++) {
            h_ap_dev[a] = b->h_dev_of[gains->ap_surface[a]];
            h_ap_f64[a] = gains->ap_normal_x[a];
            h_ap_f64[NA + a] = gains->ap_normal_y[a];
            h_ap_f64[2 * NA + a] = gains->ap_normal_z[a];
            for (int j = 0; j < 6; j++) h_ap_f64[(3 + j) * NA + a] = gains->ap_tau_coef[6 * a + j];
            h_ap_f64[9 * NA + a] = gains->ap_tau_diffuse[a];
            h_ap_f64[10 * NA + a] = gains->ap_scale[a];
        }
        build_solar_gain_tables(S, b->h_dev_of.data(), gains, gnt);
        sum.bind(gains->ap_sum, 0.0, &apertures.sum);
        for (uint32_t r : gnt.rec) in.need_gain(b, r >= (uint64_t)S);  // the solar gain arrays of the sides that receive (once each)
    }
    int upload(const heat_batch *b, const double *host_transmitted, int n_steps, const ShadesTerm &shades, const InputsTerm &in) {
        if (NA == 0) return HEAT_OK;
        SERIES_TRY(series_upload(ap_dev, h_ap_dev, "aperture tables"));
        SERIES_TRY(series_upload(ap_f64, h_ap_f64, "aperture tables"));
        SERIES_TRY(series_alloc(power, (size_t)NA, "aperture powers"));
        SERIES_TRY(sum.stage((size_t)NA, true, "aperture sums"));
        if (host_transmitted) SERIES_TRY(series_alloc(transmitted, (size_t)n_steps * NA, "transmitted powers"));
        SERIES_TRY(series_upload(rec, gnt.rec, "solar gain tables"));
        SERIES_TRY(series_upload(slice_off, gnt.slice_off.data(), gnt.rec.empty() ? 0 : gnt.slice_off.size(), "solar gain tables"));
        SERIES_TRY(series_upload(ap, gnt.ap, "solar gain tables"));
        SERIES_TRY(series_upload(share, gnt.share, "solar gain tables"));
        apertures.n = (int)NA, apertures.dev = ap_dev.p, apertures.site = b->n_sites > 1 ? b->d_site.p : nullptr;
        apertures.normal = ap_f64.p, apertures.coef = ap_f64.p + 3 * NA, apertures.tau_scale = ap_f64.p + 9 * NA;
        apertures.power = power.p, apertures.shade = shades.aperture.p, apertures.sf = shades.factors();
        view.n_receivers = (int)gnt.rec.size();
        view.rec = rec.p, view.slice_off = slice_off.p, view.ap = ap.p, view.power = power.p;
        view.share = reinterpret_cast<const double2 *>(share.p);
        view.gain[0] = in.d_gain[0].p, view.gain[1] = in.d_gain[1].p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_transmitted, hipStream_t st) { return sum.fetch(st, series_fetch(host_transmitted, transmitted, st)); }
};

// The room radiation (heat_room_radiation): the entries as CSR over the receivers (plan.hpp, RoomRadiationTables), the face node of
// every distinct emitter side and the step's emissions, the receivers' records, sum_irradiance (always uploaded), the irradiance rows.
struct RadiationTerm {
    int64_t NR = 0;
    RoomRadiationTables rrt;
    std::vector<uint32_t> h_face, h_rec;
    DevBuf<uint32_t> face, rec;                    // [NM], [NR]
    DevBuf<double> emission, factor, irradiance;   // [NM], [NE], [n_steps][NR]
    DevBuf<int32_t> off, src;                      // [NR + 1], [NE]
    Acc<double> sum;
    SeriesRoomRadiation view{};
    void prepare(heat_batch *b, heat_room_radiation *radiation, InputsTerm &in) {
        NR = radiation ? radiation->n_receivers : 0;  // (entries need a receiver: there are none without)
        if (NR == 0) return;
        const int64_t S = b->n_surf;
        build_room_radiation_tables(S, radiation, rrt);
        h_face.resize(rrt.emitter.size());
        for (size_t j = 0; j < rrt.emitter.size(); j++) {
            const int64_t side = rrt.emitter[j] >= S, q = rrt.emitter[j] - side * S;
            h_face[j] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], side ? (int)b->h_node_count[q] - 1 : 0);
        }
        h_rec.resize((size_t)NR);
        for (int64_t r = 0; r < NR; r++) {
            const int side = radiation->rc_side[r];
            h_rec[r] = (uint32_t)((int64_t)side * S + b->h_dev_of[radiation->rc_surface[r]]);
            in.need_gain(b, 2 + side);  // the long-wave gain arrays of the sides that receive (once each)
        }
        sum.bind(radiation->sum_irradiance, 0.0, &view.sum);
    }
    int upload(const double *host_irradiance, int n_steps, const InputsTerm &in) {
        if (NR == 0) return HEAT_OK;
        SERIES_TRY(series_upload(face, h_face, "room radiation tables"));
        SERIES_TRY(series_alloc(emission, h_face.size(), "emissions"));
        SERIES_TRY(series_upload(rec, h_rec, "room radiation tables"));
        SERIES_TRY(series_upload(off, rrt.off, "room radiation tables"));
        SERIES_TRY(series_upload(src, rrt.src, "room radiation tables"));
        SERIES_TRY(series_upload(factor, rrt.factor, "room radiation tables"));
        SERIES_TRY(sum.stage((size_t)NR, true, "irradiance sums"));
        if (host_irradiance) SERIES_TRY(series_alloc(irradiance, (size_t)n_steps * NR, "irradiances"));
        view.n_emitters = (int)h_face.size(), view.n_receivers = (int)NR, view.face = face.p, view.emission = emission.p;
        view.rec = rec.p, view.off = off.p, view.src = src.p, view.factor = factor.p;
        view.gain[0] = in.d_gain[2].p, view.gain[1] = in.d_gain[3].p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_irradiance, hipStream_t st) { return sum.fetch(st, series_fetch(host_irradiance, irradiance, st)); }
};

// The ambient drive (heat_ambient_drive), or one heat_batch_set_ambient: the sides' records and the back records that follow a front
// (plan.hpp, AmbientTables), the caller's lists, the mixing zones and factors only where a side mixes, sum_temperature, the ambient_t rows.
struct AmbientTerm {
    int64_t NB = 0;
    AmbientTables abt;
    std::vector<int32_t> h_zone;
    std::vector<double> h_mix;
    DevBuf<uint32_t> rec, peer;            // [N]
    DevBuf<int32_t> chan, zone;            // [N]
    DevBuf<double> gain, offset, mix, t;   // [N]; t: [n_steps][N], the setter: the temperatures [N]
    Acc<double> sum;
    SeriesAmbient view{};
    void prepare(const heat_batch *b, const int32_t *const side_kind[2], heat_ambient_drive *ambient) {
        NB = ambient ? ambient->n_sides : 0;
        if (NB == 0) return;
        build_ambient_tables(b->n_surf, b->h_dev_of.data(), side_kind, NB, ambient->surface, ambient->side, abt);
        sum.bind(ambient->sum_temperature, 0.0, &view.sum);
        bool mixes = false;
        for (int64_t i = 0; i < NB && ambient->mix_zone && !mixes; i++) mixes = ambient->mix_zone[i] >= 0;
        if (!mixes) return;
        h_zone.assign(ambient->mix_zone, ambient->mix_zone + NB);
        h_mix.assign((size_t)NB, 0.0);
        for (int64_t i = 0; i < NB; i++)
            if (h_zone[(size_t)i] >= 0) h_mix[(size_t)i] = ambient->mix[i];
    }
    int upload_tables() {
        SERIES_TRY(series_upload(rec, abt.rec, "ambient tables"));
        SERIES_TRY(series_upload(peer, abt.peer, "ambient tables"));
        view.rec = rec.p, view.peer = peer.p;
        return HEAT_OK;
    }
    int upload(const heat_ambient_drive *ambient, const double *host_t, int n_steps) {
        if (NB == 0) return HEAT_OK;
        SERIES_TRY(upload_tables());
        SERIES_TRY(series_upload(chan, ambient->chan, (size_t)NB, "ambient tables"));
        SERIES_TRY(report_array(gain, ambient->gain, (size_t)NB, true, "ambient tables"));
        SERIES_TRY(report_array(offset, ambient->offset, (size_t)NB, true, "ambient tables"));
        if (!h_zone.empty()) {
            SERIES_TRY(series_upload(zone, h_zone, "ambient tables"));
            SERIES_TRY(series_upload(mix, h_mix, "ambient tables"));
        }
        SERIES_TRY(sum.stage((size_t)NB, true, "ambient temperature sums"));
        if (host_t) SERIES_TRY(series_alloc(t, (size_t)n_steps * NB, "ambient temperatures"));
        view.n_sides = (int)NB, view.chan = chan.p, view.gain = gain.p, view.offset = offset.p, view.mix_zone = zone.p, view.mix = mix.p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_t, hipStream_t st) { return sum.fetch(st, series_fetch(host_t, t, st)); }
};

// The air paths (heat_air_paths): the list sorted by target zone with CSR offsets (plan.hpp, AirPathTables), the state bytes,
// the accumulators (always uploaded) and the path_q rows in the caller's order.
struct AirTerm {
    heat_air_paths *air = nullptr;
    int64_t NP = 0;
    AirPathTables apt;
    std::vector<uint8_t> h_state;
    DevBuf<int32_t> i32;
    DevBuf<double> f64, path_q;  // path_q: [n_steps][NP]
    DevBuf<uint8_t> state;       // [NP]
    Acc<double> sum_q;
    Acc<int64_t> steps_open, switches;
    AirPathsDev view{};
    void prepare(const heat_batch *b, heat_air_paths *air_) {
        air = air_;
        NP = air ? air->n_paths : 0;
        if (NP == 0) return;
        build_air_path_tables(b->n_zones, air, apt);
        h_state.assign((size_t)NP, 0);
        if (air->state) std::copy(air->state, air->state + NP, h_state.begin());
        sum_q.bind(air->sum_q, 0.0, &view.sum_q), steps_open.bind(air->steps_open, 0, &view.steps_open);
        switches.bind(air->switches, 0, &view.switches);
    }
    int upload(const heat_batch *b, const double *host_q, int n_steps) {
        if (NP == 0) return HEAT_OK;
        SERIES_TRY(series_upload(i32, apt.i32, "air path tables"));
        SERIES_TRY(series_upload(f64, apt.f64, "air path tables"));
        SERIES_TRY(series_upload(state, h_state, "air path states"));
        SERIES_TRY(sum_q.stage((size_t)NP, true, "air path accumulators"));
        SERIES_TRY(steps_open.stage((size_t)NP, true, "air path accumulators"));
        SERIES_TRY(switches.stage((size_t)NP, true, "air path accumulators"));
        if (host_q) SERIES_TRY(series_alloc(path_q, (size_t)n_steps * NP, "air path powers"));
        const int32_t *list = i32.p + (b->n_zones + 1);
        view.off = i32.p, view.source = list, view.temp_chan = list + NP, view.volume_chan = list + 2 * NP, view.open_chan = list + 3 * NP;
        view.orig = list + 4 * NP, view.state = state.p;
        view.volume_gain = f64.p, view.sense = f64.p + NP, view.half_band = f64.p + 2 * NP, view.min_delta = f64.p + 3 * NP;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_q, hipStream_t st) {
        if (NP == 0) return hipSuccess;
        const hipError_t e = series_fetch(air->state, state, st, series_fetch(host_q, path_q, st));
        return switches.fetch(st, steps_open.fetch(st, sum_q.fetch(st, e)));
    }
};

// The air handlers (heat_air_handlers): the branches as CSR over the units and the supply branches as CSR over the zones
// (plan.hpp, HandlerTables), the units' rows, the step's scratch (Ts per unit, m per branch), the bypass bytes, the
// accumulators (always uploaded) and the four arrays of rows in the caller's order. Nothing of it exists on the device
// without units.
struct HandlersTerm {
    heat_air_handlers *ah = nullptr;
    int64_t NU = 0, NBR = 0;
    HandlerTables aht;
    std::vector<uint8_t> h_bypass;
    DevBuf<int32_t> unit_off, u_zone, u_chan, u_orig, zone_off, z_unit, z_orig, i32;
    DevBuf<uint8_t> u_kind, bypass;
    DevBuf<double> u_gain, f64, ts, m, supply_t, recovered, coil_q, branch_q;  // the last four: [n_steps][NU] thrice, [n_steps][NBR]
    Acc<double> unit_f64[3];   // sum_recovered, sum_heating, sum_cooling
    Acc<int64_t> unit_i64[4];  // steps_bypass, switches, steps_heat_saturated, steps_cool_saturated
    Acc<double> sum_branch_q;
    HandlersDev view{};
    void prepare(const heat_batch *b, heat_air_handlers *ah_) {
        ah = ah_;
        NU = ah ? ah->n_units : 0;
        if (NU == 0) return;
        NBR = ah->n_branches;
        build_air_handler_tables(b->n_zones, ah, aht);
        h_bypass.assign((size_t)NU, 0);
        if (ah->bypass) std::copy(ah->bypass, ah->bypass + NU, h_bypass.begin());
        unit_f64[0].bind(ah->sum_recovered, 0.0, &view.sum_recovered), unit_f64[1].bind(ah->sum_heating, 0.0, &view.sum_heating);
        unit_f64[2].bind(ah->sum_cooling, 0.0, &view.sum_cooling);
        unit_i64[0].bind(ah->steps_bypass, 0, &view.steps_bypass), unit_i64[1].bind(ah->switches, 0, &view.switches);
        unit_i64[2].bind(ah->steps_heat_saturated, 0, &view.steps_heat_saturated);
        unit_i64[3].bind(ah->steps_cool_saturated, 0, &view.steps_cool_saturated);
        sum_branch_q.bind(ah->sum_branch_q, 0.0, &view.sum_branch_q);
    }
    bool supplies() const { return !aht.z_orig.empty(); }
    int upload(const double *host_supply, const double *host_recovered, const double *host_coil, const double *host_branch, int n_steps) {
        if (NU == 0) return HEAT_OK;
        SERIES_TRY(series_upload(unit_off, aht.unit_off, "air handler tables"));
        SERIES_TRY(series_upload(u_zone, aht.u_zone, "air handler tables"));
        SERIES_TRY(series_upload(u_chan, aht.u_chan, "air handler tables"));
        SERIES_TRY(series_upload(u_orig, aht.u_orig, "air handler tables"));
        SERIES_TRY(series_upload(u_kind, aht.u_kind, "air handler tables"));
        SERIES_TRY(series_upload(u_gain, aht.u_gain, "air handler tables"));
        SERIES_TRY(series_upload(zone_off, aht.zone_off, "air handler tables"));
        SERIES_TRY(series_upload(z_unit, aht.z_unit, "air handler tables"));
        SERIES_TRY(series_upload(z_orig, aht.z_orig, "air handler tables"));
        SERIES_TRY(series_upload(i32, aht.i32, "air handler tables"));
        SERIES_TRY(series_upload(f64, aht.f64, "air handler tables"));
        SERIES_TRY(series_upload(bypass, h_bypass, "air handler bypass states"));
        SERIES_TRY(series_alloc(ts, (size_t)NU, "supply temperatures"));
        SERIES_TRY(series_alloc(m, (size_t)NBR, "branch mass flows"));
        for (auto &a : unit_f64) SERIES_TRY(a.stage((size_t)NU, true, "air handler accumulators"));
        for (auto &a : unit_i64) SERIES_TRY(a.stage((size_t)NU, true, "air handler accumulators"));
        SERIES_TRY(sum_branch_q.stage((size_t)NBR, true, "air handler accumulators"));
        if (host_supply) SERIES_TRY(series_alloc(supply_t, (size_t)n_steps * NU, "supply temperatures"));
        if (host_recovered) SERIES_TRY(series_alloc(recovered, (size_t)n_steps * NU, "recovered powers"));
        if (host_coil) SERIES_TRY(series_alloc(coil_q, (size_t)n_steps * NU, "coil powers"));
        if (host_branch) SERIES_TRY(series_alloc(branch_q, (size_t)n_steps * NBR, "branch powers"));
        view.n_units = (int)NU, view.unit_off = unit_off.p, view.u_zone = u_zone.p, view.u_chan = u_chan.p, view.u_orig = u_orig.p;
        view.u_kind = u_kind.p, view.u_gain = u_gain.p, view.zone_off = zone_off.p, view.z_unit = z_unit.p, view.z_orig = z_orig.p;
        view.outdoor_chan = i32.p + AH_OUTDOOR_CHAN * NU, view.eff_chan = i32.p + AH_EFF_CHAN * NU, view.bypass_chan = i32.p + AH_BYPASS_CHAN * NU;
        view.heat_chan = i32.p + AH_HEAT_CHAN * NU, view.cool_chan = i32.p + AH_COOL_CHAN * NU;
        view.eff_gain = f64.p + AH_EFF_GAIN * NU, view.half_band = f64.p + AH_HALF_BAND * NU, view.min_delta = f64.p + AH_MIN_DELTA * NU;
        view.heat_cap = f64.p + AH_HEAT_CAP * NU, view.cool_cap = f64.p + AH_COOL_CAP * NU;
        view.ts = ts.p, view.m = m.p, view.bypass = bypass.p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_supply, double *host_recovered, double *host_coil, double *host_branch, hipStream_t st) {
        if (NU == 0) return hipSuccess;
        hipError_t e = series_fetch(host_recovered, recovered, st, series_fetch(host_supply, supply_t, st));
        e = series_fetch(ah->bypass, bypass, st, series_fetch(host_branch, branch_q, st, series_fetch(host_coil, coil_q, st, e)));
        return sum_branch_q.fetch(st, for_each_acc(unit_i64, &Acc<int64_t>::fetch, st, for_each_acc(unit_f64, &Acc<double>::fetch, st, e)));
    }
};

// The air species (heat_air_species): the sources as CSR over the (species, zone) lanes and the vents as CSR over the zones
// (plan.hpp, SpeciesTables), the rows of channels, the handlers' branch volumes in the caller's order, the step's scratch (V
// per vent), the concentrations twice — a step reads one and writes the other, `now` is the one the next step reads —, the
// accumulators and the three arrays of rows. Nothing of it exists on the device without species.
struct SpeciesTerm {
    heat_air_species *sp = nullptr;
    int64_t NSP = 0, NV = 0, L = 0;  // species, vents, lanes = NSP * Z
    SpeciesTables spt;
    DevBuf<int32_t> outdoor_chan, src_off, src_chan, vent_off, v_i32, limit_chan, occ_chan, br_chan;
    DevBuf<double> src_factor, v_f64, br_gain, vent_V, conc[2], conc_rows, vent_v, vent_q;  // the last three: [n_steps][L], [n_steps][NV] twice
    int now = 0;
    Acc<double> lane_f64[3];   // sum_conc, max_conc, excess_above
    Acc<int64_t> lane_i64[3];  // n_occupied, step_max, n_above
    Acc<double> vent_f64[2];   // sum_volume, sum_q
    Acc<int64_t> steps_saturated;
    SpeciesDev view{};
    void prepare(const heat_batch *b, const heat_air_handlers *ah, heat_air_species *sp_) {
        sp = sp_;
        NSP = sp ? sp->n_species : 0;
        if (NSP == 0) return;
        NV = sp->n_vents, L = NSP * b->n_zones;
        build_air_species_tables(b->n_zones, ah, sp, spt);
        lane_f64[0].bind(sp->sum_conc, 0.0, &view.sum_conc), lane_f64[1].bind(sp->max_conc, -std::numeric_limits<double>::infinity(), &view.max_conc);
        lane_f64[2].bind(sp->excess_above, 0.0, &view.excess_above);
        lane_i64[0].bind(sp->n_occupied, 0, &view.n_occupied), lane_i64[1].bind(sp->step_max, -1, &view.step_max);
        lane_i64[2].bind(sp->n_above, 0, &view.n_above);
        vent_f64[0].bind(sp->sum_volume, 0.0, &view.sum_volume), vent_f64[1].bind(sp->sum_q, 0.0, &view.sum_q);
        steps_saturated.bind(sp->steps_saturated, 0, &view.steps_saturated);
    }
    int upload(const double *host_conc, const double *host_v, const double *host_q, int n_steps) {
        if (NSP == 0) return HEAT_OK;
        const bool resume = sp->resume != 0;
        SERIES_TRY(series_upload(outdoor_chan, spt.outdoor_chan, "air species tables"));
        SERIES_TRY(series_upload(src_off, spt.src_off, "air species tables"));
        SERIES_TRY(series_upload(src_chan, spt.src_chan, "air species tables"));
        SERIES_TRY(series_upload(src_factor, spt.src_factor, "air species tables"));
        SERIES_TRY(series_upload(limit_chan, spt.limit_chan, "air species tables"));
        SERIES_TRY(series_upload(occ_chan, spt.occ_chan, "air species tables"));
        SERIES_TRY(series_upload(br_chan, spt.br_chan, "air species tables"));
        SERIES_TRY(series_upload(br_gain, spt.br_gain, "air species tables"));
        SERIES_TRY(series_upload(conc[0], sp->conc, (size_t)L, "concentrations"));
        SERIES_TRY(series_alloc(conc[1], (size_t)L, "concentrations"));
        if (host_conc) SERIES_TRY(series_alloc(conc_rows, (size_t)n_steps * L, "concentration rows"));
        for (auto &a : lane_f64) SERIES_TRY(a.stage((size_t)L, resume, "air species accumulators"));
        for (auto &a : lane_i64) SERIES_TRY(a.stage((size_t)L, resume, "air species accumulators"));
        view.n_species = (int)NSP, view.n_vents = (int)NV, view.outdoor_chan = outdoor_chan.p, view.src_off = src_off.p, view.src_chan = src_chan.p;
        view.src_factor = src_factor.p, view.limit_chan = limit_chan.p, view.occ_chan = occ_chan.p, view.br_chan = br_chan.p, view.br_gain = br_gain.p;
        if (NV == 0) return HEAT_OK;
        // (the vents' rows packed into two uploads: v_species, v_temp_chan, v_enable_chan, v_orig and v_min, v_max, c_lo, c_hi)
        std::vector<int32_t> h_i32;
        std::vector<double> h_f64;
        for (auto *v : {&spt.v_species, &spt.v_temp_chan, &spt.v_enable_chan, &spt.v_orig}) h_i32.insert(h_i32.end(), v->begin(), v->end());
        for (auto *v : {&spt.v_min, &spt.v_max, &spt.c_lo, &spt.c_hi}) h_f64.insert(h_f64.end(), v->begin(), v->end());
        SERIES_TRY(series_upload(vent_off, spt.vent_off, "demand vent tables"));
        SERIES_TRY(series_upload(v_i32, h_i32, "demand vent tables"));
        SERIES_TRY(series_upload(v_f64, h_f64, "demand vent tables"));
        SERIES_TRY(series_alloc(vent_V, (size_t)NV, "vent volume flows"));
        for (auto &a : vent_f64) SERIES_TRY(a.stage((size_t)NV, resume, "demand vent accumulators"));
        SERIES_TRY(steps_saturated.stage((size_t)NV, resume, "demand vent accumulators"));
        if (host_v) SERIES_TRY(series_alloc(vent_v, (size_t)n_steps * NV, "vent volume flows"));
        if (host_q) SERIES_TRY(series_alloc(vent_q, (size_t)n_steps * NV, "vent powers"));
        view.vent_off = vent_off.p, view.v_species = v_i32.p, view.v_temp_chan = v_i32.p + NV, view.v_enable_chan = v_i32.p + 2 * NV;
        view.v_orig = v_i32.p + 3 * NV, view.v_min = v_f64.p, view.v_max = v_f64.p + NV, view.c_lo = v_f64.p + 2 * NV, view.c_hi = v_f64.p + 3 * NV;
        view.vent_V = vent_V.p;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        if (NSP == 0 || sp->resume != 0) return hipSuccess;
        hipError_t e = for_each_acc(lane_i64, &Acc<int64_t>::start, st, for_each_acc(lane_f64, &Acc<double>::start, st));
        return steps_saturated.start(st, for_each_acc(vent_f64, &Acc<double>::start, st, e));
    }
    hipError_t fetch(double *host_conc, double *host_v, double *host_q, hipStream_t st) {
        if (NSP == 0) return hipSuccess;
        hipError_t e = series_fetch(host_q, vent_q, st, series_fetch(host_v, vent_v, st, series_fetch(host_conc, conc_rows, st)));
        e = series_fetch(sp->conc, conc[now], st, e);
        e = for_each_acc(lane_i64, &Acc<int64_t>::fetch, st, for_each_acc(lane_f64, &Acc<double>::fetch, st, e));
        return steps_saturated.fetch(st, for_each_acc(vent_f64, &Acc<double>::fetch, st, e));
    }
};

// The openings (heat_openings): the tables in the caller's order (plan.hpp, OpeningTables), the accumulators (uploaded on
// resume, else started on the device) and the opening_v rows. Nothing of it exists on the device without openings.
struct OpeningsTerm {
    heat_openings *op = nullptr;
    int64_t NO = 0;
    OpeningTables opt;
    DevBuf<int32_t> i32;          // [kOpeningI32Rows][NO]
    DevBuf<double> f64, v;        // [kOpeningF64Rows][NO]; v: [n_steps][NO]
    Acc<double> acc_f64[2];       // sum_v, max_v
    Acc<int64_t> step_max;
    OpeningsDev view{};
    void prepare(heat_openings *op_) {
        op = op_;
        NO = op ? op->n_openings : 0;
        if (NO == 0) return;
        build_opening_tables(op, opt);
        acc_f64[0].bind(op->sum_v, 0.0, &view.sum_v), acc_f64[1].bind(op->max_v, -std::numeric_limits<double>::infinity(), &view.max_v);
        step_max.bind(op->step_max, -1, &view.step_max);
    }
    int upload(const double *host_v, int n_steps) {
        if (NO == 0) return HEAT_OK;
        const bool resume = op->resume != 0;
        SERIES_TRY(series_upload(i32, opt.i32, "opening tables"));
        SERIES_TRY(series_upload(f64, opt.f64, "opening tables"));
        for (auto &a : acc_f64) SERIES_TRY(a.stage((size_t)NO, resume, "opening accumulators"));
        SERIES_TRY(step_max.stage((size_t)NO, resume, "opening accumulators"));
        if (host_v) SERIES_TRY(series_alloc(v, (size_t)n_steps * NO, "opening volume flows"));
        view.n_openings = (int)NO;
        view.zone_a = i32.p + OP_ZONE_A * NO, view.zone_b = i32.p + OP_ZONE_B * NO, view.temp_chan = i32.p + OP_TEMP_CHAN * NO;
        view.wind_chan = i32.p + OP_WIND_CHAN * NO, view.frac_chan = i32.p + OP_FRAC_CHAN * NO, view.out_chan = i32.p + OP_OUT_CHAN * NO;
        view.area = f64.p + OP_AREA * NO, view.cw = f64.p + OP_CW * NO, view.cs = f64.p + OP_CS * NO, view.ca = f64.p + OP_CA * NO;
        view.c0 = f64.p + OP_C0 * NO;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        return NO > 0 && op->resume == 0 ? step_max.start(st, for_each_acc(acc_f64, &Acc<double>::start, st)) : hipSuccess;
    }
    hipError_t fetch(double *host_v, hipStream_t st) {
        if (NO == 0) return hipSuccess;
        return step_max.fetch(st, for_each_acc(acc_f64, &Acc<double>::fetch, st, series_fetch(host_v, v, st)));
    }
};

// The controllers (heat_controllers): the tables in the caller's order (plan.hpp, ControllerTables) with the sensed nodes
// resolved to their places in the device's T buffer, the state (always on the device: uploaded on resume where the caller
// holds it, else zeroed there), the accumulators (uploaded on resume, else started on the device) and the control_u and
// control_out rows. Nothing of it exists on the device without controllers.
struct ControllersTerm {
    heat_controllers *ct = nullptr;
    int64_t NCT = 0;
    ControllerTables ctt;
    DevBuf<int32_t> i32;          // [kControllerI32Rows][NCT]
    DevBuf<double> f64, u, out;   // [kControllerF64Rows][NCT]; u, out: [n_steps][NCT]
    DevBuf<double> integral;
    DevBuf<uint8_t> tripped;
    Acc<double> acc_f64[2];       // sum_u, sum_out
    Acc<int64_t> acc_i64[3];      // steps_on, steps_sat, trips
    ControllersDev view{};
    // A sensed node's place in T: its slot of the caller's state through the resolver the probes use, then the probes' placement
    // (the device's node layout is packed: the descriptor's numbering does not index T).
    int prepare(heat_batch *b, const SeriesModel &m, heat_controllers *ct_) {
        ct = ct_;
        NCT = ct ? ct->n_controllers : 0;
        if (NCT == 0) return HEAT_OK;
        bool resolved = true;
        build_controller_tables(m, ct, [&](int64_t q, int node) {
            int kind = 0, n = 0;
            int64_t index = 0;
            uint8_t buf = 0;
            uint32_t idx = 0;
            if (!b->resolver->resolve(b->h_first_slot[q] + node, kind, index, n) || kind != PROBE_NODE || index != q || n != node) {
                resolved = false;
                return (uint32_t)0;
            }
            ProbesTerm::place(b, kind, index, n, buf, idx);
            if ((size_t)idx >= b->d_T.n) resolved = false;
            return resolved ? idx : (uint32_t)0;
        }, ctt);
        if (!resolved) return fail(HEAT_E_SIZE, "controllers: a sensed node's slot is not resolved to a node of the batch");
        acc_f64[0].bind(ct->sum_u, 0.0, &view.sum_u), acc_f64[1].bind(ct->sum_out, 0.0, &view.sum_out);
        acc_i64[0].bind(ct->steps_on, 0, &view.steps_on), acc_i64[1].bind(ct->steps_sat, 0, &view.steps_sat);
        acc_i64[2].bind(ct->trips, 0, &view.trips);
        return HEAT_OK;
    }
    int upload(const double *host_u, const double *host_out, int n_steps) {
        if (NCT == 0) return HEAT_OK;
        const bool resume = ct->resume != 0;
        SERIES_TRY(series_upload(i32, ctt.i32, "controller tables"));
        SERIES_TRY(series_upload(f64, ctt.f64, "controller tables"));
        SERIES_TRY(series_alloc(integral, (size_t)NCT, "controller state", resume ? ct->integral : nullptr));
        SERIES_TRY(series_alloc(tripped, (size_t)NCT, "controller state", resume ? ct->tripped : nullptr));
        for (auto &a : acc_f64) SERIES_TRY(a.stage((size_t)NCT, resume, "controller accumulators"));
        for (auto &a : acc_i64) SERIES_TRY(a.stage((size_t)NCT, resume, "controller accumulators"));
        if (host_u) SERIES_TRY(series_alloc(u, (size_t)n_steps * NCT, "controller signals"));
        if (host_out) SERIES_TRY(series_alloc(out, (size_t)n_steps * NCT, "controller outputs"));
        view.n_controllers = (int)NCT;
        view.sense_kind = i32.p + CT_SENSE_KIND * NCT, view.set_chan = i32.p + CT_SET_CHAN * NCT, view.action = i32.p + CT_ACTION * NCT;
        view.en_chan = i32.p + CT_EN_CHAN * NCT, view.lim_kind = i32.p + CT_LIM_KIND * NCT, view.out_chan = i32.p + CT_OUT_CHAN * NCT;
        view.sense_at = reinterpret_cast<const uint32_t *>(i32.p + CT_SENSE_AT * NCT);
        view.lim_at = reinterpret_cast<const uint32_t *>(i32.p + CT_LIM_AT * NCT);
        view.kp = f64.p + CT_KP * NCT, view.ki = f64.p + CT_KI * NCT, view.bias = f64.p + CT_BIAS * NCT, view.out_lo = f64.p + CT_OUT_LO * NCT;
        view.out_hi = f64.p + CT_OUT_HI * NCT, view.lim_hi = f64.p + CT_LIM_HI * NCT, view.lim_lo = f64.p + CT_LIM_LO * NCT;
        view.integral = integral.p, view.tripped = tripped.p;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        if (NCT == 0) return hipSuccess;
        const bool resume = ct->resume != 0;
        hipError_t e = hipSuccess;
        if (!(resume && ct->integral)) e = hipMemsetAsync(integral.p, 0, (size_t)NCT * sizeof(double), st);
        if (e == hipSuccess && !(resume && ct->tripped)) e = hipMemsetAsync(tripped.p, 0, (size_t)NCT, st);
        return resume ? e : for_each_acc(acc_i64, &Acc<int64_t>::start, st, for_each_acc(acc_f64, &Acc<double>::start, st, e));
    }
    hipError_t fetch(double *host_u, double *host_out, hipStream_t st) {
        if (NCT == 0) return hipSuccess;
        hipError_t e = series_fetch(host_out, out, st, series_fetch(host_u, u, st));
        e = series_fetch(ct->tripped, tripped, st, series_fetch(ct->integral, integral, st, e));
        return for_each_acc(acc_i64, &Acc<int64_t>::fetch, st, for_each_acc(acc_f64, &Acc<double>::fetch, st, e));
    }
};

// The air networks (heat_air_networks): the tables sorted by width class (plan.hpp, NetworkTables), the pressures (always on the
// device: uploaded on resume where the caller holds them, else zeroed there), the accumulators (uploaded on resume, else
// started on the device) and the link_q, node_p and net_iters rows, all in the caller's order. Nothing of it exists on the
// device without networks.
struct NetworksTerm {
    heat_air_networks *nw = nullptr;
    int64_t NW = 0, NN = 0, NK = 0;
    NetworkTables nt;
    DevBuf<int32_t> net_i32, node_i32, inc, link_i32, iters;   // iters: [n_steps][NW]
    DevBuf<double> net_f64, node_f64, link_f64, pressure, q, p; // q: [n_steps][NK]; p: [n_steps][NN]
    Acc<double> acc_f64[3];       // sum_ab, sum_ba, max_res
    Acc<int64_t> acc_i64[2];      // iters_sum, unconverged
    NetworksDev view{};
    int prepare(int64_t n_zones, int32_t n_channels, heat_air_networks *nw_) {
        nw = nw_;
        NW = nw ? nw->n_networks : 0;
        if (NW == 0) return HEAT_OK;
        NN = nw->n_nodes, NK = nw->n_links;
        build_network_tables(nw, nt);
        // (every index a lane uses lies inside its array: a kernel that wrote out of bounds would not fail alone)
        SERIES_TRY(check_network_tables(n_zones, n_channels, nw, nt, heat::last_error()));
        acc_f64[0].bind(nw->sum_ab, 0.0, &view.sum_ab), acc_f64[1].bind(nw->sum_ba, 0.0, &view.sum_ba), acc_f64[2].bind(nw->max_res, 0.0, &view.max_res);
        acc_i64[0].bind(nw->iters_sum, 0, &view.iters_sum), acc_i64[1].bind(nw->unconverged, 0, &view.unconverged);
        return HEAT_OK;
    }
    int upload(const double *host_q, const double *host_p, const int32_t *host_iters, int n_steps) {
        if (NW == 0) return HEAT_OK;
        const bool resume = nw->resume != 0;
        SERIES_TRY(series_upload(net_i32, nt.net_i32, "network tables"));
        SERIES_TRY(series_upload(net_f64, nt.net_f64, "network tables"));
        SERIES_TRY(series_upload(node_i32, nt.node_i32, "network tables"));
        SERIES_TRY(series_upload(node_f64, nt.node_f64, "network tables"));
        SERIES_TRY(series_upload(inc, nt.inc, "network tables"));
        SERIES_TRY(series_upload(link_i32, nt.link_i32, "network tables"));
        SERIES_TRY(series_upload(link_f64, nt.link_f64, "network tables"));
        SERIES_TRY(series_alloc(pressure, (size_t)NN, "network pressures", resume ? nw->pressure : nullptr));
        for (size_t a = 0; a < 2; a++) SERIES_TRY(acc_f64[a].stage((size_t)NK, resume, "network accumulators"));
        SERIES_TRY(acc_f64[2].stage((size_t)NW, resume, "network accumulators"));
        for (auto &a : acc_i64) SERIES_TRY(a.stage((size_t)NW, resume, "network accumulators"));
        if (host_q) SERIES_TRY(series_alloc(q, (size_t)n_steps * NK, "network link flows"));
        if (host_p) SERIES_TRY(series_alloc(p, (size_t)n_steps * NN, "network node pressures"));
        if (host_iters) SERIES_TRY(series_alloc(iters, (size_t)n_steps * NW, "network iteration counts"));
        for (int c = 0; c <= kNetworkClasses; c++) view.class_start[c] = nt.class_start[c];
        view.n_nodes = (int)NN, view.n_links = (int)NK;
        view.net_id = net_i32.p + NW_ID * NW, view.net_n = net_i32.p + NW_N * NW, view.net_node0 = net_i32.p + NW_NODE0 * NW;
        view.net_max_iter = net_i32.p + NW_MAX_ITER * NW, view.net_tol = net_f64.p + NW_TOL * NW, view.net_g_min = net_f64.p + NW_G_MIN * NW;
        view.node_id = node_i32.p + ND_ID * NN, view.node_zone = node_i32.p + ND_ZONE * NN, view.node_src_chan = node_i32.p + ND_SRC_CHAN * NN;
        view.node_inc0 = node_i32.p + ND_INC0 * NN, view.node_inc_n = node_i32.p + ND_INC_N * NN, view.node_src_gain = node_f64.p, view.inc = inc.p;
        view.zone_a = link_i32.p + LK_ZONE_A * NK, view.zone_b = link_i32.p + LK_ZONE_B * NK, view.la = link_i32.p + LK_LA * NK;
        view.lb = link_i32.p + LK_LB * NK, view.temp_chan = link_i32.p + LK_TEMP_CHAN * NK, view.wp_chan = link_i32.p + LK_WP_CHAN * NK;
        view.frac_chan = link_i32.p + LK_FRAC_CHAN * NK, view.out_ab = link_i32.p + LK_OUT_AB * NK, view.out_ba = link_i32.p + LK_OUT_BA * NK;
        view.c = link_f64.p + LK_C * NK, view.gh = link_f64.p + LK_GH * NK, view.p_lin = link_f64.p + LK_P_LIN * NK;
        view.s_lin = link_f64.p + LK_S_LIN * NK, view.wp_gain = link_f64.p + LK_WP_GAIN * NK;
        view.pressure = pressure.p;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        if (NW == 0) return hipSuccess;
        const bool resume = nw->resume != 0;
        hipError_t e = hipSuccess;
        if (!(resume && nw->pressure)) e = hipMemsetAsync(pressure.p, 0, (size_t)NN * sizeof(double), st);
        return resume ? e : for_each_acc(acc_i64, &Acc<int64_t>::start, st, for_each_acc(acc_f64, &Acc<double>::start, st, e));
    }
    hipError_t fetch(double *host_q, double *host_p, int32_t *host_iters, hipStream_t st) {
        if (NW == 0) return hipSuccess;
        hipError_t e = series_fetch(host_iters, iters, st, series_fetch(host_p, p, st, series_fetch(host_q, q, st)));
        e = series_fetch(nw->pressure, pressure, st, e);
        return for_each_acc(acc_i64, &Acc<int64_t>::fetch, st, for_each_acc(acc_f64, &Acc<double>::fetch, st, e));
    }
};

// The anisotropic sky (heat_sky_aniso): the coefficient table as given, beside the record table, and the bands of the three
// consumers — the sides' per DEVICE surface, the apertures' and the shades' in the caller's order as their tables are; zeros
// where the caller gave none. Absent (every pointer NULL) without aniso: the isotropic kernels are launched.
struct AnisoTerm {
    const heat_sky_aniso *an = nullptr;
    std::vector<double> h_side;
    DevBuf<SkyCoef> coef;                  // [n_steps][n_sites]
    DevBuf<double> side, aperture, shade;  // [2][S], [NA], [NS]
    void prepare(heat_batch *b, const heat_sky_aniso *an_, unsigned sky_bits) {
        an = an_;
        if (!an || !(sky_bits & 3)) return;
        h_side.assign(2 * (size_t)b->n_surf, 0.0);
        if (an->front_band) to_device_order(b, an->front_band, h_side.data());
        if (an->back_band) to_device_order(b, an->back_band, h_side.data() + b->n_surf);
    }
    static int band(DevBuf<double> &buf, const double *src, int64_t n, const char *what) {
        if (n <= 0) return HEAT_OK;
        if (src) return series_upload(buf, src, (size_t)n, what);
        return series_upload(buf, std::vector<double>((size_t)n, 0.0), what);
    }
    int upload(const heat_batch *b, const heat_series *s, int64_t NA, int64_t NS) {
        if (!an) return HEAT_OK;
        SERIES_TRY(series_upload(coef, reinterpret_cast<const SkyCoef *>(an->coef), (size_t)s->n_steps * b->n_sites, "sky coefficients"));
        SERIES_TRY(series_upload(side, h_side, "side bands"));
        SERIES_TRY(band(aperture, an->aperture_band, NA, "aperture bands"));
        SERIES_TRY(band(shade, an->shade_band, NS, "shade bands"));
        return HEAT_OK;
    }
};
static_assert(sizeof(SkyCoef) == sizeof(heat_sky_coef) && sizeof(heat_sky_coef) == 16, "SkyCoef mirrors heat_sky_coef");

// Comfort (heat_comfort): the entries as CSR over the sensors with their face nodes and weights (plan.hpp, ComfortTables), the
// sensors' rows, the step's operative temperatures, the accumulators (uploaded on resume, else started on the device) and the
// operative / mrt rows; with a control sensor the control sensor of every zone and the step's control temperatures. Nothing of
// it exists on the device without sensors.
struct ComfortTerm {
    heat_comfort *cf = nullptr;
    int64_t NF = 0;
    ComfortTables cft;
    DevBuf<int32_t> off, i32, ctl;                    // [NF + 1], [kComfortI32Rows][NF], [Z]
    DevBuf<uint32_t> face;                            // [NE]
    DevBuf<double> weight, air_weight, top, control_T, operative, mrt;  // [NE], [NF], [NF], [Z], [n_steps][NF] twice
    Acc<double> f64[6];   // sum_operative, min_operative, max_operative, deg_below, deg_above, max_above
    Acc<int64_t> i64[6];  // n_occupied, step_min, step_max, n_below, n_above, step_max_above
    SeriesComfort view{};
    void prepare(const heat_batch *b, heat_comfort *cf_) {
        cf = cf_;
        NF = cf ? cf->n_sensors : 0;
        if (NF == 0) return;
        const double inf = std::numeric_limits<double>::infinity();
        build_comfort_tables(b->n_zones, cf, b->h_node_tile_base.data(), b->h_node_geom.data(), b->h_first_slot.data(), b->h_node_count.data(), cft);
        f64[0].bind(cf->sum_operative, 0.0, &view.sum_operative), f64[1].bind(cf->min_operative, inf, &view.min_operative);
        f64[2].bind(cf->max_operative, -inf, &view.max_operative), f64[3].bind(cf->deg_below, 0.0, &view.deg_below);
        f64[4].bind(cf->deg_above, 0.0, &view.deg_above), f64[5].bind(cf->max_above, -inf, &view.max_above);
        i64[0].bind(cf->n_occupied, 0, &view.n_occupied), i64[1].bind(cf->step_min, -1, &view.step_min);
        i64[2].bind(cf->step_max, -1, &view.step_max), i64[3].bind(cf->n_below, 0, &view.n_below);
        i64[4].bind(cf->n_above, 0, &view.n_above), i64[5].bind(cf->step_max_above, -1, &view.step_max_above);
    }
    int upload(const heat_batch *b, const double *host_operative, const double *host_mrt, int n_steps) {
        if (NF == 0) return HEAT_OK;
        const bool resume = cf->resume != 0;
        SERIES_TRY(series_upload(off, cft.off, "comfort tables"));
        SERIES_TRY(series_upload(face, cft.face, "comfort tables"));
        SERIES_TRY(series_upload(weight, cft.weight, "comfort tables"));
        SERIES_TRY(series_upload(i32, cft.i32, "comfort tables"));
        SERIES_TRY(series_upload(air_weight, cft.air_weight, "comfort tables"));
        SERIES_TRY(series_alloc(top, (size_t)NF, "operative temperatures"));
        if (cft.any_control) {
            SERIES_TRY(series_upload(ctl, cft.ctl_sensor, "comfort tables"));
            SERIES_TRY(series_alloc(control_T, (size_t)b->n_zones, "control temperatures"));
        }
        if (host_operative) SERIES_TRY(series_alloc(operative, (size_t)n_steps * NF, "operative temperatures"));
        if (host_mrt) SERIES_TRY(series_alloc(mrt, (size_t)n_steps * NF, "mean radiant temperatures"));
        for (auto &a : f64) SERIES_TRY(a.stage((size_t)NF, resume, "comfort accumulators"));
        for (auto &a : i64) SERIES_TRY(a.stage((size_t)NF, resume, "comfort accumulators"));
        view.n_sensors = (int)NF, view.off = off.p, view.face = face.p, view.weight = weight.p;
        view.zone = i32.p + CF_ZONE * NF, view.occ_chan = i32.p + CF_OCC_CHAN * NF, view.lo_chan = i32.p + CF_LO_CHAN * NF;
        view.hi_chan = i32.p + CF_HI_CHAN * NF, view.air_weight = air_weight.p, view.top = top.p;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        return NF > 0 && cf->resume == 0 ? for_each_acc(i64, &Acc<int64_t>::start, st, for_each_acc(f64, &Acc<double>::start, st)) : hipSuccess;
    }
    hipError_t fetch(double *host_operative, double *host_mrt, hipStream_t st) {
        if (NF == 0) return hipSuccess;
        const hipError_t e = series_fetch(host_mrt, mrt, st, series_fetch(host_operative, operative, st));
        return for_each_acc(i64, &Acc<int64_t>::fetch, st, for_each_acc(f64, &Acc<double>::fetch, st, e));
    }
};

// What heat_batch_march_series_call takes (the eleven positional entry points fill what they have) and, beside it, the comfort
// term and its two arrays of rows (heat_batch_march_series_comfort), the air handlers with their four
// (heat_batch_march_series_handlers), the air species with their three (heat_batch_march_series_species), the openings with
// their one (heat_batch_march_series_openings) and the controllers with their two (heat_batch_march_series_controllers);
// filled by field name. no_trace_ok: a NULL trace records none.
struct SeriesCall {
    const heat_series *s = nullptr;
    const heat_sky *sky = nullptr;
    const heat_sky_aniso *aniso = nullptr;
    const heat_shades *shades = nullptr;
    const heat_solar_gains *gains = nullptr;
    const heat_zone_loads *l = nullptr;
    heat_air_paths *air = nullptr;
    heat_ideal_loads *il = nullptr;
    heat_series_report *r = nullptr;
    double *trace = nullptr, *applied = nullptr, *ideal_q = nullptr, *transmitted = nullptr, *path_q = nullptr, *sunlit = nullptr;
    heat_room_radiation *radiation = nullptr;
    double *irradiance = nullptr;
    heat_ambient_drive *ambient = nullptr;
    double *ambient_t = nullptr;
    heat_blinds *blinds = nullptr;
    double *position = nullptr, *blind_incident = nullptr;
    heat_comfort *comfort = nullptr;
    double *operative = nullptr, *mrt = nullptr;
    heat_air_handlers *handlers = nullptr;
    double *supply_t = nullptr, *recovered = nullptr, *coil_q = nullptr, *branch_q = nullptr;
    heat_air_species *species = nullptr;
    double *conc_rows = nullptr, *vent_v = nullptr, *vent_q = nullptr;
    heat_openings *openings = nullptr;
    double *opening_v = nullptr;
    heat_controllers *controllers = nullptr;
    double *control_u = nullptr, *control_out = nullptr;
    heat_air_networks *networks = nullptr;
    double *link_q = nullptr, *node_p = nullptr;
    int32_t *net_iters = nullptr;
    int32_t *failed_step = nullptr;
    bool no_trace_ok = false;
};

}  // namespace

extern "C" {

// heat_batch_march_series*: the table of contents of a series march. A term that is absent (its argument NULL, or naming
// nothing: loads without a term, no ideal load, no mode bit, no aperture, no path, no shade, no receiver, no driven side) is
// the series without it: the same launches. no_trace_ok: a NULL trace means "record none" instead of a refusal.
static int march_series_impl(heat_batch *b, const SeriesCall &c) {
    if (c.failed_step) *c.failed_step = -1;
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    const heat_series *s = c.s;
    // ---- everything that needs no device (heat_series_check's checks, on the batch's own copies of the slots) ----
    SeriesModel m;
    m.n_surfaces = b->n_surf, m.n_zones = b->n_zones;
    m.first_node_slot = b->h_first_slot.data(), m.node_count = b->h_node_count.data();
    for (int a = 0; a < 4; a++) m.out_slot[a] = b->h_out_slots[a].data();
    m.zone_slot = b->h_zone_slot_h.data();
    if (!b->resolver) b->resolver = new SlotResolver(m);
    std::vector<ResolvedSlot> group_entry;
    std::vector<int32_t> load_of_zone;
    const int32_t *const side_kind[2] = {b->h_kind[0].data(), b->h_kind[1].data()};
    SkyTerm sky;
    int rc;
    if ((rc = check_series(m, *b->resolver, b->n_sites, s, heat::last_error()))) return rc;
    if ((rc = check_zone_loads(b->n_zones, s->n_channels, c.l, heat::last_error()))) return rc;
    if ((rc = check_series_report(*b->resolver, c.l, c.r, heat::last_error(), &group_entry))) return rc;
    if ((rc = check_ideal_loads(b->n_zones, s->n_channels, c.il, heat::last_error(), &load_of_zone))) return rc;
    if ((rc = check_sky(b->n_surf, s, c.sky, heat::last_error(), &sky.bits))) return rc;
    if (b->n_ranks > 1) return fail(HEAT_E_INVALID_ARG, "a sharded batch (n_ranks = %d) cannot march a series", b->n_ranks);
    // (behind the shard's refusal: the gains number the surfaces of the caller's model, a shard holds some of them)
    if ((rc = check_solar_gains(b->n_surf, s, c.sky, c.gains, heat::last_error()))) return rc;
    if ((rc = check_shades(b->n_surf, s, c.sky, c.gains, c.shades, heat::last_error()))) return rc;
    if ((rc = check_sky_aniso(b->n_surf, s, c.sky, c.gains, c.shades, c.aniso, heat::last_error()))) return rc;
    if ((rc = check_blinds(b->n_zones, s, c.shades, c.blinds, heat::last_error()))) return rc;
    if ((rc = check_air_paths(b->n_zones, s->n_channels, c.air, heat::last_error()))) return rc;
    if ((rc = check_room_radiation(b->n_surf, s, c.sky, c.radiation, heat::last_error()))) return rc;
    if ((rc = check_ambient(b->n_surf, side_kind, b->n_zones, s, c.ambient, heat::last_error()))) return rc;
    if ((rc = check_comfort(b->n_surf, b->n_zones, s, c.comfort, heat::last_error()))) return rc;
    if ((rc = check_air_handlers(b->n_zones, s->n_channels, c.handlers, heat::last_error()))) return rc;
    if ((rc = check_air_species(b->n_zones, s->n_channels, c.species, heat::last_error()))) return rc;
    if ((rc = check_openings(b->n_zones, s->n_channels, c.openings, heat::last_error()))) return rc;
    if ((rc = check_controllers(m, s->n_channels, c.openings, c.controllers, heat::last_error()))) return rc;
    if ((rc = check_air_networks(b->n_zones, s->n_channels, c.openings, c.controllers, c.networks, heat::last_error()))) return rc;
    const int64_t S = b->n_surf, Z = b->n_zones, P = s->n_probes, n_sites = b->n_sites;
    const int n_steps = s->n_steps, n_sub = s->n_sub, NC = s->n_channels;
    if (!c.trace && !c.no_trace_ok && (int64_t)n_steps * P > 0) return fail(HEAT_E_INVALID_ARG, "trace is NULL");
    if (n_steps == 0) return HEAT_OK;
    if ((rc = select_device(b))) return rc;
    if ((rc = grow_weather(b, n_sub))) return rc;  // (once, before the first step: the pointers a captured graph holds stay valid)
    b->n_weather = n_sub;
    // ---- the terms: host tables first; on the device for the duration of the call, freed on every return path behind the drain ----
    // The schedules: a step's weather records exactly as heat_batch_set_weather lays them out in d_weather (site-major,
    // weather_cap apart); the zone terms as rows of [a0[Z] | b0[Z]] as k_begin_march reads them (no rows given: one of zeros)
    const size_t cap = b->weather_cap, n_rec = n_sub > 0 ? (size_t)(n_sites - 1) * cap + (size_t)n_sub : 0;
    const int zrows = std::max(s->n_zone_term_steps, 1);
    std::vector<StepWeather> h_w((size_t)n_steps * n_rec, StepWeather{0.0, 0.0, 0.0, 0.0});
    std::vector<double> h_zab((size_t)zrows * 2 * Z, 0.0);
    for (int k = 0; k < n_steps; k++)
        for (int64_t st = 0; st < n_sites; st++)
            for (int i = 0; i < n_sub; i++)
                h_w[(size_t)k * n_rec + st * cap + i] = to_step_weather(s->weather[((size_t)k * n_sub + i) * n_sites + st]);
    for (int64_t i = 0; i < (int64_t)zrows * Z && s->n_zone_term_steps > 0; i++) {
        if (s->zone_a0) h_zab[(size_t)(i / Z * 2 * Z + i % Z)] = s->zone_a0[i];
        if (s->zone_b0) h_zab[(size_t)((i / Z * 2 + 1) * Z + i % Z)] = s->zone_b0[i];
    }
    DevBuf<StepWeather> d_w;
    DevBuf<double> d_zab, d_channel;
    InputsTerm in; ProbesTerm probes; LoadsTerm loads; ReportTerm report; IdealTerm ideal;
    ShadesTerm shades; BlindsTerm blinds; GainsTerm gains; RadiationTerm radiation; AmbientTerm ambient; AirTerm air; AnisoTerm aniso;
    ComfortTerm comfort;
    HandlersTerm handlers;
    SpeciesTerm species;
    OpeningsTerm openings;
    ControllersTerm controllers;
    NetworksTerm networks;
    in.prepare(b, s);
    sky.prepare(b, c.sky, in);
    gains.prepare(b, c.gains, in);
    shades.prepare(b, c.shades, sky.bits);
    blinds.prepare(c.blinds, shades.NS);
    aniso.prepare(b, c.aniso, sky.bits);
    radiation.prepare(b, c.radiation, in);
    ambient.prepare(b, side_kind, c.ambient);
    if ((rc = probes.prepare(b, s))) return rc;
    report.prepare(b, c.r, P, group_entry);
    loads.prepare(b, c.l);
    ideal.prepare(c.il, load_of_zone);
    air.prepare(b, c.air);
    comfort.prepare(b, c.comfort);
    handlers.prepare(b, c.handlers);
    species.prepare(b, c.handlers, c.species);
    openings.prepare(c.openings);
    if ((rc = controllers.prepare(b, m, c.controllers))) return rc;
    if ((rc = networks.prepare(b->n_zones, s->n_channels, c.networks))) return rc;
    const int64_t NT = loads.NT, NI = ideal.NI, NA = gains.NA, NS = shades.NS, NR = radiation.NR, NB = ambient.NB, NP = air.NP, G = report.G;
    const int64_t NL = blinds.NL, NF = comfort.NF, NU = handlers.NU, NBR = handlers.NBR, NSP = species.NSP, NV = species.NV;
    const int64_t NO = openings.NO, NCT = controllers.NCT, NNW = networks.NW;
    SeriesDrain drain{b};
    if ((rc = series_upload(d_w, h_w, "weather schedule"))) return rc;
    if ((rc = series_upload(d_zab, h_zab, "zone terms"))) return rc;
    if ((rc = series_upload(d_channel, s->channel, (size_t)n_steps * NC, "channel table"))) return rc;
    if ((rc = in.upload())) return rc;
    if ((rc = probes.upload(c.trace, n_steps))) return rc;
    if ((rc = loads.upload(c.applied, n_steps))) return rc;
    if ((rc = report.upload(n_steps, probes, loads))) return rc;
    if ((rc = ideal.upload(b, c.ideal_q, n_steps))) return rc;
    if ((rc = sky.upload(b, s, c.sky, sky.bits || NA > 0 || NS > 0, in))) return rc;
    if ((rc = shades.upload(c.shades, NA, c.sunlit, n_steps, NL > 0, sky))) return rc;
    if ((rc = blinds.upload(shades, c.position, c.blind_incident, n_steps))) return rc;
    if ((rc = gains.upload(b, c.transmitted, n_steps, shades, in))) return rc;
    if ((rc = aniso.upload(b, s, NA, NS))) return rc;
    if ((rc = radiation.upload(c.irradiance, n_steps, in))) return rc;
    if ((rc = ambient.upload(c.ambient, c.ambient_t, n_steps))) return rc;
    if ((rc = air.upload(b, c.path_q, n_steps))) return rc;
    if ((rc = comfort.upload(b, c.operative, c.mrt, n_steps))) return rc;
    if ((rc = handlers.upload(c.supply_t, c.recovered, c.coil_q, c.branch_q, n_steps))) return rc;
    if ((rc = species.upload(c.conc_rows, c.vent_v, c.vent_q, n_steps))) return rc;
    if ((rc = openings.upload(c.opening_v, n_steps))) return rc;
    if ((rc = controllers.upload(c.control_u, c.control_out, n_steps))) return rc;
    if ((rc = networks.upload(c.link_q, c.node_p, c.net_iters, n_steps))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the uploads went through the null stream; the batch's streams do not wait for it)
    HIP_TRY(report.start(b->stream));
    HIP_TRY(ideal.start(b->stream));
    HIP_TRY(comfort.start(b->stream));
    HIP_TRY(species.start(b->stream));
    HIP_TRY(openings.start(b->stream));
    HIP_TRY(controllers.start(b->stream));
    HIP_TRY(networks.start(b->stream));
    // what the thermostats, the air paths' e and the blinds sense: the zone temperatures, or with a control sensor the step's Tc
    const double *control_T = comfort.control_T.p ? comfort.control_T.p : b->d_zone_T.p;
    double *mirror = b->direct_runs.empty() ? nullptr : b->d_state.p;
    // ---- the steps, enqueued without waiting: controllers -> openings (the two writers of the step's row of d_channel; everything behind reads it,
    // and a captured graph holds the body of the march only, which reads no channel) -> head -> comfort -> control temperatures -> zone loads -> thermostat statistics -> air paths -> air handlers -> air species -> ambient drive ->
    // driven inputs -> shades -> blinds -> sky -> solar gains -> room radiation -> the body of a march call of n_sub -> probes -> report ----
    for (int k = 0; k < n_steps; k++) {
        if (NCT > 0)
            launch_series_controllers(controllers.view, row(d_channel, k, NC), b->d_T.p, b->d_zone_T.p, row(controllers.u, k, NCT), row(controllers.out, k, NCT),
                                      b->stream);
        if (NO > 0) launch_series_openings(openings.view, row(d_channel, k, NC), b->d_zone_T.p, row(openings.v, k, NO), c.openings->step_base + k, b->stream);
        // (the networks behind the openings: one launch per width class present, the third writer of the step's row)
        if (NNW > 0)
            launch_series_networks(networks.view, row(d_channel, k, NC), b->d_zone_T.p, row(networks.q, k, networks.NK), row(networks.p, k, networks.NN),
                                   row(networks.iters, k, NNW), b->stream);
        const double *channel = row(d_channel, k, NC);
        const SkyRecord *record = row(sky.record, k, n_sites);
        const SkyCoef *coef = row(aniso.coef, k, n_sites);  // (nullptr without aniso: the isotropic kernels)
        // (the powers of the step: a row of the applied buffer, or one row of scratch where the caller takes none)
        double *applied = loads.applied.p ? row(loads.applied, k, NT) : report.applied_row.p;
        launch_begin_march(row(d_w, k, (int64_t)n_rec), b->d_weather.p, n_sub, (int)n_rec, row(d_zab, std::min(k, zrows - 1), 2 * Z), b->d_zone_a0.p, b->d_zone_b0.p, (int)Z, b->d_step.p, b->stream);
        if (NF > 0) {
            launch_series_comfort(comfort.view, channel, b->d_T.p, b->d_zone_T.p, row(comfort.operative, k, NF), row(comfort.mrt, k, NF),
                                  c.comfort->step_base + k, b->stream);
            if (comfort.control_T.p) launch_series_control_T((int)Z, comfort.ctl.p, comfort.top.p, b->d_zone_T.p, comfort.control_T.p, b->stream);
        }
        if (loads.on)
            launch_series_zone_loads((int)Z, loads.view, channel, control_T, b->d_zone_a0.p, b->d_zone_b0.p, applied, b->d_flags.p, b->stream);
        if (report.th_stats) launch_series_th_stats((int)NT, report.th, loads.mode.p, applied, b->stream);
        if (NP > 0)
            launch_series_air_paths((int)Z, air.view, channel, b->d_zone_T.p, control_T, b->d_zone_a0.p, b->d_zone_b0.p, row(air.path_q, k, NP), b->d_flags.p,
                                    b->stream);
        if (NU > 0) {
            double *branch_row = row(handlers.branch_q, k, NBR);
            launch_series_handler_units(handlers.view, channel, b->d_zone_T.p, row(handlers.supply_t, k, NU), row(handlers.recovered, k, NU),
                                        row(handlers.coil_q, k, NU), branch_row, b->stream);
            if (handlers.supplies())
                launch_series_handler_supply((int)Z, handlers.view, b->d_zone_T.p, b->d_zone_a0.p, b->d_zone_b0.p, branch_row, b->d_flags.p, b->stream);
        }
        if (NSP > 0) {
            const double *conc = species.conc[species.now].p;
            if (NV > 0)
                launch_series_vents((int)Z, species.view, channel, b->d_zone_T.p, conc, b->d_zone_a0.p, b->d_zone_b0.p, row(species.vent_v, k, NV),
                                    row(species.vent_q, k, NV), b->d_flags.p, b->stream);
            launch_series_species((int)Z, species.view, loads.on ? &loads.view : nullptr, NP > 0 ? &air.view : nullptr,
                                  NU > 0 ? &handlers.view : nullptr, channel, b->d_zone_vol.p, (double)n_sub * b->dt, conc,
                                  species.conc[species.now ^ 1].p, row(species.conc_rows, k, species.L), c.species->step_base + k, b->stream);
            species.now ^= 1;
        }
        if (NB > 0) launch_series_ambient(ambient.view, channel, b->d_zone_T.p, b->d_side_const.p, row(ambient.t, k, NB), b->stream);
        if (in.driven)
            launch_series_inputs((int)S, channel, in.view, b->d_T.p, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, b->stream);
        if (NS > 0) launch_series_shading(record, shades.view, row(shades.sunlit, k, NS), b->stream);
        if (NL > 0)
            launch_series_blinds(record, blinds.view, channel, control_T, row(blinds.position, k, NL), row(blinds.incident, k, NL), coef,
                                 aniso.shade.p, b->stream);
        if (sky.bits) launch_series_sky((int)S, record, sky.view, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, coef, aniso.side.p, b->stream);
        if (NA > 0) {
            launch_series_apertures(record, gains.apertures, row(gains.transmitted, k, NA), coef, aniso.aperture.p, b->stream);
            launch_series_solar_gains((int)S, gains.view, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, b->stream);
        }
        if (NR > 0) {
            launch_series_emission(radiation.view, b->d_T.p, b->stream);
            launch_series_room_radiation((int)S, radiation.view, channel, b->d_side_dyn.p, b->sl, mirror, row(radiation.irradiance, k, NR),
                                         b->stream);
        }
        if (NI > 0) {
            launch_series_ideal_begin(ideal.view, channel, b->stream);
            rc = march_body_ideal(b, n_sub, ideal.view);
        } else {
            rc = march_body(b, n_sub);
        }
        if (rc) return rc;
        if (NI > 0) launch_series_ideal_end(ideal.view, row(ideal.q, k, NI), c.il->step_base + k, b->stream);
        // (without a trace: no probe is copied, lane 0 still watches the failure flags)
        launch_series_probe(probes.trace.p ? P : 0, probes.buf.p, probes.idx.p, b->d_T.p, b->d_side_out.p, b->d_zone_T.p,
                            row(probes.trace, k, P), b->d_flags.p, probes.failed.p, k, b->stream);
        if (report.q_stats) {  // (a report that asks nothing of its quantities launches nothing here)
            launch_series_groups(report.groups, b->d_T.p, b->d_side_out.p, b->d_zone_T.p, b->stream);
            launch_series_stats(report.stats, b->d_T.p, b->d_side_out.p, b->d_zone_T.p, row(report.group_trace, k, G), c.r->step_base + k,
                                b->stream);
        }
    }
    HIP_TRY(hipGetLastError());
    // ---- one wait: the rows, the accumulators and the record of the first failure travel at the end of the stream's work ----
    int first_failed[5] = {-1, 0, 0, 0, 0};
    HIP_TRY(probes.fetch(c.trace, b->stream));
    HIP_TRY(loads.fetch(c.l, c.applied, b->stream));
    HIP_TRY(report.fetch(b->stream));
    HIP_TRY(ideal.fetch(c.ideal_q, b->stream));
    HIP_TRY(gains.fetch(c.transmitted, b->stream));
    HIP_TRY(air.fetch(c.path_q, b->stream));
    HIP_TRY(shades.fetch(c.sunlit, b->stream));
    HIP_TRY(blinds.fetch(c.position, c.blind_incident, b->stream));
    HIP_TRY(radiation.fetch(c.irradiance, b->stream));
    HIP_TRY(ambient.fetch(c.ambient_t, b->stream));
    HIP_TRY(comfort.fetch(c.operative, c.mrt, b->stream));
    HIP_TRY(handlers.fetch(c.supply_t, c.recovered, c.coil_q, c.branch_q, b->stream));
    HIP_TRY(species.fetch(c.conc_rows, c.vent_v, c.vent_q, b->stream));
    HIP_TRY(openings.fetch(c.opening_v, b->stream));
    HIP_TRY(controllers.fetch(c.control_u, c.control_out, b->stream));
    HIP_TRY(networks.fetch(c.link_q, c.node_p, c.net_iters, b->stream));
    HIP_TRY(hipMemcpyAsync(first_failed, probes.failed.p, sizeof first_failed, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (first_failed[0] < 0) return HEAT_OK;  // (the flags were clear after the last step: nothing to report)
    // A numerical failure: reported as heat_batch_synchronize reports it, from the flags as they were after the step that
    // set them (the steps enqueued behind it marched on and may have added to them).
    if (c.failed_step) *c.failed_step = first_failed[0];
    HIP_TRY(hipMemcpy(b->d_flags.p, first_failed + 1, 4 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return heat_batch_synchronize(b);
}

int heat_batch_march_series(heat_batch *b, const heat_series *s, double *trace, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.trace = trace, c.failed_step = failed_step;
    return march_series_impl(b, c);
}

int heat_batch_march_series_loads(heat_batch *b, const heat_series *s, const heat_zone_loads *l, double *trace, double *applied,
                                  int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.trace = trace, c.applied = applied, c.failed_step = failed_step;
    return march_series_impl(b, c);
}

int heat_batch_march_series_report(heat_batch *b, const heat_series *s, const heat_zone_loads *l, heat_series_report *r, double *trace,
                                   double *applied, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.r = r, c.trace = trace, c.applied = applied, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_ideal(heat_batch *b, const heat_series *s, const heat_zone_loads *l, heat_ideal_loads *il,
                                  heat_series_report *r, double *trace, double *applied, double *ideal_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied, c.ideal_q = ideal_q;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_sky(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_zone_loads *l, heat_ideal_loads *il,
                                heat_series_report *r, double *trace, double *applied, double *ideal_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied, c.ideal_q = ideal_q;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_gains(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_solar_gains *gains,
                                  const heat_zone_loads *l, heat_ideal_loads *il, heat_series_report *r, double *trace, double *applied,
                                  double *ideal_q, double *transmitted, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.gains = gains, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied;
    c.ideal_q = ideal_q, c.transmitted = transmitted, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_air(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_solar_gains *gains,
                                const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il, heat_series_report *r, double *trace,
                                double *applied, double *ideal_q, double *transmitted, double *path_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace, c.applied = applied;
    c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_shaded(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                   const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                   heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                   double *path_q, double *sunlit, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_radiation(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                      const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                      heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                      double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                      int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_ambient(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                    const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                    heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                    double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                    heat_ambient_drive *ambient, double *ambient_t, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.ambient = ambient, c.ambient_t = ambient_t, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_blinds(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                   const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                   heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                   double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                   heat_ambient_drive *ambient, double *ambient_t, heat_blinds *blinds, double *position,
                                   double *blind_incident, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.ambient = ambient, c.ambient_t = ambient_t, c.blinds = blinds, c.position = position;
    c.blind_incident = blind_incident, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

// heat_batch_march_series_call, heat_batch_march_series_comfort, heat_batch_march_series_handlers,
// heat_batch_march_series_species, heat_batch_march_series_openings and heat_batch_march_series_controllers: the struct's fields
// by name, then the comfort term, then the air handlers, the air species, the openings and the controllers (`more`: what the
// last four add, or nullptr).
static int march_series_call(heat_batch *b, const heat_series_call *call, heat_comfort *comfort, double *operative, double *mrt,
                             const SeriesCall *more = nullptr) {
    if (const int rc = check_series_call(call, heat::last_error())) return rc;  // (a struct of another size is not read further)
    SeriesCall c;
    if (more) c = *more;
    c.comfort = comfort, c.operative = operative, c.mrt = mrt; c.s = call->s, c.sky = call->sky, c.aniso = call->aniso, c.shades = call->shades, c.gains = call->gains, c.l = call->l;
    c.air = call->air, c.il = call->il, c.r = call->r, c.radiation = call->radiation, c.ambient = call->ambient, c.blinds = call->blinds;
    c.trace = call->trace, c.applied = call->applied, c.ideal_q = call->ideal_q, c.transmitted = call->transmitted, c.path_q = call->path_q;
    c.sunlit = call->sunlit, c.irradiance = call->irradiance, c.ambient_t = call->ambient_t, c.position = call->position;
    c.blind_incident = call->blind_incident, c.failed_step = call->failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_call(heat_batch *b, const heat_series_call *call) { return march_series_call(b, call, nullptr, nullptr, nullptr); }

int heat_batch_march_series_comfort(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt) {
    return march_series_call(b, call, c, operative, mrt);
}

int heat_batch_march_series_handlers(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                     heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    return march_series_call(b, call, c, operative, mrt, &more);
}

int heat_batch_march_series_species(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                    heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                    heat_air_species *sp, double *conc_rows, double *vent_v, double *vent_q) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    more.species = sp, more.conc_rows = conc_rows, more.vent_v = vent_v, more.vent_q = vent_q;
    return march_series_call(b, call, c, operative, mrt, &more);
}

int heat_batch_march_series_openings(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                     heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                     heat_air_species *sp, double *conc_rows, double *vent_v, double *vent_q, heat_openings *op,
                                     double *opening_v) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    more.species = sp, more.conc_rows = conc_rows, more.vent_v = vent_v, more.vent_q = vent_q, more.openings = op, more.opening_v = opening_v;
    return march_series_call(b, call, c, operative, mrt, &more);
}

int heat_batch_march_series_controllers(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                        heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                        heat_air_species *sp, double *conc_rows, double *vent_v, double *vent_q, heat_openings *op,
                                        double *opening_v, heat_controllers *ct, double *control_u, double *control_out) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    more.species = sp, more.conc_rows = conc_rows, more.vent_v = vent_v, more.vent_q = vent_q, more.openings = op, more.opening_v = opening_v;
    more.controllers = ct, more.control_u = control_u, more.control_out = control_out;
    return march_series_call(b, call, c, operative, mrt, &more);
}

int heat_batch_march_series_networks(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                     heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                     heat_air_species *sp, double *conc_rows, double *vent_v, double *vent_q, heat_openings *op,
                                     double *opening_v, heat_controllers *ct, double *control_u, double *control_out, heat_air_networks *nw,
                                     double *link_q, double *node_p, int32_t *net_iters) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    more.species = sp, more.conc_rows = conc_rows, more.vent_v = vent_v, more.vent_q = vent_q, more.openings = op, more.opening_v = opening_v;
    more.controllers = ct, more.control_u = control_u, more.control_out = control_out;
    more.networks = nw, more.link_q = link_q, more.node_p = node_p, more.net_iters = net_iters;
    return march_series_call(b, call, c, operative, mrt, &more);
}

// The ambient temperature of the listed sides from the next march on: k_series_ambient with the temperatures as its row
// (lane i takes row[i]; no gain, offset or mix), on the batch's stream behind earlier work. The tables and the values are
// per-call device buffers: the call waits for its own kernel before it frees them, so the caller's arrays are free too.
int heat_batch_set_ambient(heat_batch *b, int64_t n, const int64_t *surface, const uint8_t *side, const double *temperature) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    // ---- everything that needs no device ----
    // (a shard holds some of the caller's surfaces under numbers of its own: out of scope, as for the series)
    if (b->n_ranks > 1) return fail(HEAT_E_INVALID_ARG, "a sharded batch (n_ranks = %d) cannot set ambient temperatures", b->n_ranks);
    if (n > 0 && !temperature) return fail(HEAT_E_INVALID_ARG, "entry 0: temperature is NULL (count %lld)", (long long)n);
    const int32_t *const side_kind[2] = {b->h_kind[0].data(), b->h_kind[1].data()};
    int rc = check_ambient_sides(b->n_surf, side_kind, n, surface, side, "entry", heat::last_error());
    if (rc) return rc;
    if (n == 0) return HEAT_OK;
    AmbientTerm abd;
    build_ambient_tables(b->n_surf, b->h_dev_of.data(), side_kind, n, surface, side, abd.abt);
    rc = select_device(b);
    if (rc) return rc;
    SeriesDrain drain{b};
    if ((rc = abd.upload_tables())) return rc;
    if ((rc = series_upload(abd.t, temperature, (size_t)n, "ambient temperatures"))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the uploads went through the null stream; the batch's streams do not wait for it)
    abd.view.n_sides = (int)n;
    launch_series_ambient(abd.view, abd.t.p, b->d_zone_T.p, b->d_side_const.p, nullptr, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    return HEAT_OK;
}

}  // extern "C"
