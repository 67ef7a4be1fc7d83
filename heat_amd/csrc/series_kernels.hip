// series_kernels.hip — gfx950 kernels of the series layer (heat_batch_march_series: series.hip drives them): what a step does
// around the march — one lane per item, none of them tuned by register count or by instruction. The march itself, the zone
// kernels and k_begin_march / k_set_step are kernels.hip's; the device helpers both files use are device_math.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "series_kernels.hpp"

namespace heat {

// ---------------------------------------------------------------------------
// Series march (heat_batch_march_series, batch.hip): what the caller does between two ThermalModel::march calls, done on the
// device from schedules uploaded once. The head of a step is k_begin_march itself, reading the step's weather records and
// zone terms from the device-resident schedules instead of the pinned staging buffers.
//
// k_series_inputs — the driven inputs of one step, one lane per device surface. `row` is the step's row of the channel
// table (a few KB: cache resident); the value of an input is gain x channel, for a long-wave input plus
// sigma (T + 273.15)^4 of the surface's own face node as it is at the start of the step where asked
// (validate_wall_heat_transfer.rs:689-699). From there on it is k_inputs_compact: the same clamps, the same conversion, the
// raw value into the state mirror where the batch keeps one. A field whose channel is -1 is NOT written (it keeps what the
// last upload or series put there): a side with both fields driven is one 16-byte store, with one an 8-byte store, a
// surface with no driven input leaves after reading its four channel numbers.
__device__ __forceinline__ void series_side(int side, int d, int S, int c_solar, int c_ir, int own, const double *__restrict__ row,
                                            const SeriesInputs &in, const double *__restrict__ T,
                                            const double *__restrict__ side_alpha, SideDyn *__restrict__ dyn, const SlotArrays &sl,
                                            double *__restrict__ mirror) {
    if ((c_solar & c_ir) < 0) return;  // both -1
    const int64_t rec = (int64_t)side * S + d;
    double solar = 0.0, rad_t = 0.0;
    if (c_solar >= 0) {
        double raw = row[c_solar];
        if (in.gain[side]) raw *= in.gain[side][d];
        if (mirror != nullptr) mirror[(side ? sl.solar_b : sl.solar_f)[d]] = raw;
        solar = (side ? clamp_solar_back(raw) : clamp_solar_front(raw)) * side_alpha[rec];
    }
    if (c_ir >= 0) {
        double raw = row[c_ir];
        if (in.gain[2 + side]) raw *= in.gain[2 + side][d];
        if ((own >> side) & 1) {
            const double tk = T[in.face[rec]] + 273.15;
            const double tk2 = tk * tk;
            raw += kSigma * (tk2 * tk2);
        }
        if (mirror != nullptr) mirror[(side ? sl.ir_b : sl.ir_f)[d]] = raw;
        rad_t = ir_to_rad_temperature(raw);
    }
    if (c_solar >= 0 && c_ir >= 0) reinterpret_cast<double2 *>(dyn)[rec] = make_double2(solar, rad_t);
    else if (c_solar >= 0) dyn[rec].solar = solar;
    else dyn[rec].rad_t = rad_t;
}

__global__ void __launch_bounds__(256)
k_series_inputs(int n_surf, const double *__restrict__ row, SeriesInputs in, const double *__restrict__ T,
                const double *__restrict__ side_alpha, SideDyn *__restrict__ dyn, SlotArrays sl, double *__restrict__ mirror) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    const int S = n_surf;
    if (d >= S) return;
    const int c_sf = in.chan[d], c_sb = in.chan[(int64_t)S + d], c_if = in.chan[2 * (int64_t)S + d], c_ib = in.chan[3 * (int64_t)S + d];
    if ((c_sf & c_sb & c_if & c_ib) < 0) return;  // every one of them -1: nothing of this surface is driven
    const int own = in.own_face ? in.own_face[d] : 0;
    series_side(0, d, S, c_sf, c_if, own, row, in, T, side_alpha, dyn, sl, mirror);
    series_side(1, d, S, c_sb, c_ib, own, row, in, T, side_alpha, dyn, sl, mirror);
}

// k_series_probe — the tail of a step: one lane per probe copies a value of the device state (a node temperature, a
// coefficient or flow of a SideOut record, a zone temperature: buffer and index resolved by the host) into the step's row
// of the trace. The first time lane 0 finds the failure flags set it notes the step and the flags as they are then —
// fail_step[0] = step, [1..4] = flags[0..3] (kinds, first failing surface: report_failure) — so that the host reports what a
// march call that ended with this step would have reported, whatever the steps after it add.
__global__ void __launch_bounds__(256)
k_series_probe(int64_t n_probes, const uint8_t *__restrict__ buf, const uint32_t *__restrict__ idx, const double *__restrict__ T,
               const SideOut *__restrict__ out, const double *__restrict__ zone_T, double *__restrict__ trace_row,
               const int *__restrict__ flags, int *__restrict__ fail_step, int step) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 && fail_step[0] < 0 && flags[0] != 0) {
        fail_step[0] = step;
        for (int q = 0; q < 4; q++) fail_step[1 + q] = flags[q];
    }
    if (p >= n_probes) return;
    const int b = buf[p];
    const double *base = b == kProbeBufT ? T : (b == kProbeBufOut ? reinterpret_cast<const double *>(out) : zone_T);
    trace_row[p] = base[idx[p]];
}

// k_series_zone_loads — the zone loads of one step (heat_zone_loads, include/heat_amd.h), between the step's head and its
// driven inputs: one lane per zone walks the zone's gains, flows and thermostats (CSR ranges of lists sorted by zone, the
// caller's order kept inside a zone) and adds them to the a0 / b0 the head has just written; a zone without terms leaves
// after reading its offsets. `row` is the step's row of the channel table (a few KB: cache resident). A thermostat reads its
// sensor zone's temperature as the step before left it — nothing in this kernel writes zone_T — and belongs to the lane
// of its target zone alone: its mode byte and its element of `applied` have one writer.
// Every product and sum is one rounded operation, in the order the header gives: the host applying the same rule between
// march calls reproduces the bits. Hence no contraction, and the air properties are written out here: device_math.hpp's
// air_heat_capacity is compiled where a + b * c contracts to a fused multiply-add.
// A term that turns a zone's a0 or b0 into NaN (a NaN channel value, say) is reported as the zone's failure here: the zone
// update keeps the temperature of a zone whose b is NaN (model.rs:662-668, |b| > 1e-9 is false) and would hide it.
#pragma clang fp contract(off)
__global__ void __launch_bounds__(256)
k_series_zone_loads(int n_zones, ZoneLoadsDev zl, const double *__restrict__ row, const double *__restrict__ zone_T,
                    double *__restrict__ a0, double *__restrict__ b0, double *__restrict__ applied_row, int *__restrict__ flags) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n_zones) return;
    const int32_t *og = zl.off, *of = zl.off + (n_zones + 1), *ot = zl.off + 2 * (n_zones + 1);
    const int g0 = og[z], g1 = og[z + 1], f0 = of[z], f1 = of[z + 1], t0 = ot[z], t1 = ot[z + 1];
    if (g0 == g1 && f0 == f1 && t0 == t1) return;
    double a = a0[z], b = b0[z];
    const bool clean = a == a && b == b;
    for (int i = g0; i < g1; i++) {  // model.rs:500-516
        const double p = zl.gain_factor[i] * row[zl.gain_chan[i]];
        a = a + p;
    }
    for (int i = f0; i < f1; i++) {  // model.rs:522-544
        const double v = zl.flow_volume_gain[i] * row[zl.flow_volume_chan[i]];
        const double t_in = row[zl.flow_temp_chan[i]];
        const double tk = t_in + 273.15;
        const double rho = 101325. * 28.97 / (8314.46261815324 * tk);  // gas.rs:175-179
        const double cp = 1002.7370 + 1.2324e-2 * tk;                  // gas.rs:49,165-167
        const double m = (rho * v) * cp;
        const double mt = m * t_in;
        a = a + mt;
        b = b + m;
    }
    for (int i = t0; i < t1; i++) {
        const int orig = zl.th_orig[i];
        const int hc = zl.th_heat_chan[i], cc = zl.th_cool_chan[i];
        const double ts = zone_T[zl.th_sensor[i]], d = zl.th_half_band[i];
        int mode = zl.th_mode[orig];
        if (hc >= 0) {
            const double h = row[hc];
            if (ts < h - d) mode = 1;
            else if (mode == 1 && ts > h + d) mode = 0;
        }
        if (mode != 1 && cc >= 0) {
            const double c = row[cc];
            if (ts > c + d) mode = 2;
            else if (mode == 2 && ts < c - d) mode = 0;
        }
        const double power = mode == 1 ? zl.th_heat_power[i] : (mode == 2 ? -zl.th_cool_power[i] : 0.0);
        a = a + power;
        zl.th_mode[orig] = (uint8_t)mode;
        if (applied_row != nullptr) applied_row[orig] = power;
    }
    a0[z] = a;
    b0[z] = b;
    if (clean && (a != a || b != b)) report_failure(flags, FLAG_NAN_ZONE, (unsigned int)z);
}

// k_series_shading — the sunlit fraction of every shade in one step (heat_shades, include/heat_amd.h), behind k_series_inputs
// and before k_series_sky: one lane per shade. A lane reads its site's 64-byte record (of which it uses the sun vector), its
// 19 rows of the shade table (structure of arrays: a wavefront reads lines) and, where it has a horizon profile, one tan2
// element; it stores f for the shaded sides and apertures of k_series_sky / k_series_apertures to gather, and into the step's
// row of `sunlit` where the caller takes one. The header's rule, every line one rounded operation in the order written, hence
// no contraction; min and max are written as the comparisons the header gives, so that a NaN has one outcome. No atomics,
// no LDS.
__device__ __forceinline__ double shade_max(double a, double b) { return b > a ? b : a; }  // (the FIRST operand where false)
__device__ __forceinline__ double shade_min(double a, double b) { return b < a ? b : a; }

__global__ void __launch_bounds__(256)
k_series_shading(const SkyRecord *__restrict__ records, SeriesShades sh, double *__restrict__ sunlit_row) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = sh.n;
    if (j >= sh.n) return;
    const SkyRecord &r = records[sh.site[j]];
    const double sx = r.sun_x, sy = r.sun_y, sz = r.sun_z;
    const double *const t = sh.tab + j;
    const double c = (t[SH_NX * n] * sx + t[SH_NY * n] * sy) + t[SH_NZ * n] * sz;
    const double us = (t[SH_UX * n] * sx + t[SH_UY * n] * sy) + t[SH_UZ * n] * sz;
    const double vs = (t[SH_VX * n] * sx + t[SH_VY * n] * sy) + t[SH_VZ * n] * sz;
    const double W = t[SH_W * n], H = t[SH_H * n];
    // overhang
    const double drop = (t[SH_OD * n] * vs) / c;
    double s = drop - t[SH_OG * n];
    s = shade_max(s, 0.0);
    s = shade_min(s, H);
    const double fv = vs > 0.0 ? (H - s) / H : 1.0;
    // fins
    const double ap = (t[SH_PD * n] * us) / c;
    double wp = ap - t[SH_PG * n];
    wp = shade_max(wp, 0.0);
    wp = shade_min(wp, W);
    const double nu = -us;
    const double an = (t[SH_ND * n] * nu) / c;
    double wn = an - t[SH_NG * n];
    wn = shade_max(wn, 0.0);
    wn = shade_min(wn, W);
    const double sw = us > 0.0 ? wp : (us < 0.0 ? wn : 0.0);
    const double fh = (W - sw) / W;
    double f = fv * fh;
    const int p = sh.horizon[j];
    if (p >= 0) {
        const double ax = fabs(sx), ay = fabs(sy);
        const double T = 0.41421356237309503;
        const int m = (int)(ay > T * ax) + (int)(ay > ax) + (int)(T * ay > ax);
        const int sector = sx >= 0.0 ? (sy >= 0.0 ? m : 15 - m) : (sy >= 0.0 ? 7 - m : 8 + m);  // in [0, 16) whatever the sun holds
        const double h2 = sx * sx + sy * sy;
        const double z2 = sz * sz;
        const bool lit = sz > 0.0 && z2 > sh.tan2[16 * (int64_t)p + sector] * h2;
        if (!lit) f = 0.0;
    }
    if (!(c > 0.0)) f = 0.0;
    sh.f[j] = f;
    if (sunlit_row != nullptr) sunlit_row[j] = f;
}

// The circumsolar ratio of heat_sky_aniso: cos(incidence) over the zenith cosine held at cos 85 deg, one division; 0 on a
// plane the sun is behind and with the sun at or below the horizon. A NaN makes every comparison false.
__device__ __forceinline__ double aniso_rb(double c, double sun_z) {
#pragma clang fp contract(off)
    const double Z0 = 0.08715574274765817;
    const bool up = sun_z > 0.0;
    const double zb = sun_z > Z0 ? sun_z : Z0;
    return (c > 0.0 && up) ? c / zb : 0.0;
}

// k_series_blinds — the effective factors of every shade in one step (heat_blinds, include/heat_amd.h), behind
// k_series_shading and before k_series_sky: one lane per SHADE. Neighbouring lanes read neighbouring elements of
// blind_of_shade, of f and of five rows of the shade table (the normal and the two constant factors), and store neighbouring
// elements of the three effective arrays k_series_sky / k_series_apertures gather from. A lane whose shade carries no blind
// stores plain copies. The others gather their blind's rows of the blind table (structure of arrays in the caller's blind
// order: where the shades are not in that order the gather is scattered, over a table of 64 bytes a blind), form the
// irradiance on the shade's plane from the record of the shade's site and apply the header's rule, every line one rounded
// operation in the order written, hence no contraction; min and max are shade_max / shade_min. A blind rides on one shade:
// its state byte, accumulators and output elements have one writer. Nothing on the step's head writes the zone temperatures:
// every zone is read as it was at the start of the step. No atomics, no LDS.
// ANISO (heat_sky_aniso): the lane also loads the 16-byte coefficient pair of the shade's site and the shade's band, and I
// is the anisotropic rule of a shaded side; the instantiation without it is the kernel as it was.
template <bool ANISO>
__global__ void __launch_bounds__(256)
k_series_blinds(const SkyRecord *__restrict__ records, SeriesBlinds bl, const double *__restrict__ row, const double *__restrict__ zone_T,
                double *__restrict__ position_row, double *__restrict__ incident_row, const SkyCoef *__restrict__ coef,
                const double *__restrict__ band) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = bl.n_shades;
    if (j >= bl.n_shades) return;
    const double f = bl.f[j], fd = bl.tab[SH_FD * n + j], fg = bl.tab[SH_FG * n + j];
    const int i = bl.blind_of_shade[j];
    if (i < 0) {  // no blind: the consumers read what they read without blinds
        bl.eff_f[j] = f;
        bl.eff_diffuse[j] = fd;
        bl.eff_ground[j] = fg;
        return;
    }
    const SkyRecord &r = records[bl.site[j]];
    const double nx = bl.tab[SH_NX * n + j], ny = bl.tab[SH_NY * n + j], nz = bl.tab[SH_NZ * n + j];
    const double c = (nx * r.sun_x + ny * r.sun_y) + nz * r.sun_z;
    const double fs = 0.5 + 0.5 * nz, fgv = 0.5 - 0.5 * nz;
    double bm = c > 0.0 ? r.beam * c : 0.0;
    double I;
    if (ANISO) {
        const SkyCoef q = coef[bl.site[j]];
        const double rb = aniso_rb(c, r.sun_z);
        const double iso = 1.0 - q.circ;
        const double cs = (r.diffuse * q.circ) * rb;
        double sun = bm + cs;
        double dv = (r.diffuse * fs) * iso;
        const double hv = (r.diffuse * q.horiz) * band[j];
        dv = dv + hv;
        double gv = r.ground * fgv;
        sun = sun * f;
        dv = dv * fd;
        gv = gv * fg;
        I = (sun + dv) + gv;
    } else {
        bm = bm * f;
        const double dv = (r.diffuse * fs) * fd;
        const double gv = (r.ground * fgv) * fg;
        I = (bm + dv) + gv;
    }
    const int pc = bl.pos_chan[i];
    double p;
    bool switched = false;
    if (pc >= 0) {  // scheduled
        p = row[pc];
        p = shade_max(p, 0.0);
        p = shade_min(p, 1.0);
    } else {        // controlled
        const int ec = bl.enable_chan[i], z = bl.zone[i];
        const bool enabled = ec < 0 || row[ec] > 0.0;
        bool hot = true, cool = false;
        if (z >= 0) {
            const double set = row[bl.set_chan[i]], d = bl.half_band[i], T = zone_T[z];
            const double hi = set + d;
            const double lo = set - d;
            hot = T > hi;
            cool = T < lo;
        }
        const int before = bl.state[i];
        int state = before;
        if (!enabled) state = 0;
        else if (I > bl.irr_close[i] && hot) state = 1;
        else if (state == 1 && (I < bl.irr_open[i] || cool)) state = 0;
        switched = state != before;
        if (switched) bl.state[i] = (uint8_t)state;
        p = (double)state;
    }
    const double q = 1.0 - p;
    const double pb = p * bl.beam_closed[i];
    const double kb = q + pb;
    const double pd = p * bl.diffuse_closed[i];
    const double kd = q + pd;
    const double pg = p * bl.ground_closed[i];
    const double kg = q + pg;
    bl.eff_f[j] = f * kb;
    bl.eff_diffuse[j] = fd * kd;
    bl.eff_ground[j] = fg * kg;
    if (position_row != nullptr) position_row[i] = p;
    if (incident_row != nullptr) incident_row[i] = I;
    if (bl.sum_position != nullptr) bl.sum_position[i] = bl.sum_position[i] + p;
    if (bl.steps_closed != nullptr && p > 0.0) bl.steps_closed[i] = bl.steps_closed[i] + 1;
    if (bl.switches != nullptr && switched) bl.switches[i] = bl.switches[i] + 1;
}

// k_series_sky — the sky-driven inputs of one step (heat_sky, include/heat_amd.h), behind k_series_inputs and before the
// body: one lane per device surface. A lane whose mode byte is 0 leaves after reading it; the others read their site's
// 64-byte record of the step (the planner keeps the surfaces of a site together: a wavefront mostly reads one line) and
// their normal, and form the incident irradiance of the sides asked for by the header's rule — every product and sum one
// rounded operation in the order written, hence no contraction: the host applying the same rule (heat_amd/sky.py) between
// march calls reproduces the bits. From the raw value on it is the tail of series_side, restated: the mirror, the shared
// clamps and long-wave conversion, one 16-byte store when both fields of a side are sky-driven, else 8 bytes. An input has
// one source (check_sky): a field k_series_inputs has written is not written here.
// ANISO (heat_sky_aniso): a lane also loads its site's 16-byte coefficient pair, and a solar side its band; the solar value
// is the anisotropic rule, shaded or not. The instantiation without it is the kernel as it was.
template <bool ANISO>
__device__ __forceinline__ void sky_side(int side, int d, int S, bool m_solar, bool m_ir, double nx, double ny, double nz,
                                         const SkyRecord &r, const SeriesSky &sky, const double *__restrict__ side_alpha,
                                         SideDyn *__restrict__ dyn, const SlotArrays &sl, double *__restrict__ mirror,
                                         const SkyCoef &q, const double *__restrict__ band) {
#pragma clang fp contract(off)
    if (!(m_solar || m_ir)) return;
    const int64_t rec = (int64_t)side * S + d;
    const double fs = 0.5 + 0.5 * nz, fg = 0.5 - 0.5 * nz;
    double solar = 0.0, rad_t = 0.0;
    if (m_solar) {
        const double c = (nx * r.sun_x + ny * r.sun_y) + nz * r.sun_z;
        double bm = c > 0.0 ? r.beam * c : 0.0;
        const int j = sky.shade != nullptr ? sky.shade[rec] : -1;  // (a kernel argument: without shades the branch is wave-uniform)
        double v;
        if (ANISO) {
            const double rb = aniso_rb(c, r.sun_z);
            const double iso = 1.0 - q.circ;
            const double cs = (r.diffuse * q.circ) * rb;
            double sun = bm + cs;
            double dv = (r.diffuse * fs) * iso;
            const double hv = (r.diffuse * q.horiz) * band[rec];
            dv = dv + hv;
            double gv = r.ground * fg;
            if (j >= 0) {  // heat_shades: the sun's part times the step's sunlit fraction, the other two times their factors
                sun = sun * sky.sf.f[j];
                dv = dv * sky.sf.diffuse[j];
                gv = gv * sky.sf.ground[j];
            }
            v = (sun + dv) + gv;
        } else if (j >= 0) {  // heat_shades: the beam times the step's sunlit fraction, the other two parts times their constant factors
            bm = bm * sky.sf.f[j];
            const double dv = (r.diffuse * fs) * sky.sf.diffuse[j];
            const double gv = (r.ground * fg) * sky.sf.ground[j];
            v = (bm + dv) + gv;
        } else {
            v = (bm + r.diffuse * fs) + r.ground * fg;
        }
        if (sky.gain[side]) v = v * sky.gain[side][d];
        if (mirror != nullptr) mirror[(side ? sl.solar_b : sl.solar_f)[d]] = v;
        solar = (side ? clamp_solar_back(v) : clamp_solar_front(v)) * side_alpha[rec];
    }
    if (m_ir) {
        double v = r.ir_sky * fs + r.ir_ground * fg;
        if (sky.gain[2 + side]) v = v * sky.gain[2 + side][d];
        if (mirror != nullptr) mirror[(side ? sl.ir_b : sl.ir_f)[d]] = v;
        rad_t = ir_to_rad_temperature(v);
    }
    if (m_solar && m_ir) reinterpret_cast<double2 *>(dyn)[rec] = make_double2(solar, rad_t);
    else if (m_solar) dyn[rec].solar = solar;
    else dyn[rec].rad_t = rad_t;
}

template <bool ANISO>
__global__ void __launch_bounds__(256)
k_series_sky(int n_surf, const SkyRecord *__restrict__ records, SeriesSky sky, const double *__restrict__ side_alpha,
             SideDyn *__restrict__ dyn, SlotArrays sl, double *__restrict__ mirror, const SkyCoef *__restrict__ coef,
             const double *__restrict__ band) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    const int S = n_surf;
    if (d >= S) return;
    const int m = sky.mode[d];
    if (m == 0) return;  // nothing of this surface comes from the sky
    const int site = sky.site ? sky.site[d] : 0;
    const SkyRecord r = records[site];
    SkyCoef q{0.0, 0.0};
    if (ANISO && (m & 3)) q = coef[site];  // (read by the solar sides alone)
    const double nx = sky.normal[d], ny = sky.normal[(int64_t)S + d], nz = sky.normal[2 * (int64_t)S + d];
    sky_side<ANISO>(0, d, S, m & 1, m & 4, nx, ny, nz, r, sky, side_alpha, dyn, sl, mirror, q, band);
    sky_side<ANISO>(1, d, S, m & 2, m & 8, -nx, -ny, -nz, r, sky, side_alpha, dyn, sl, mirror, q, band);
}

// k_series_apertures — the power every window transmits in one step (heat_solar_gains, include/heat_amd.h), behind
// k_series_sky: one lane per aperture. A lane reads its site's 64-byte record, its normal, six coefficients, the
// hemispherical transmittance and the scale (structure of arrays: a wavefront reads lines), and applies the header's rule —
// every product and sum one rounded operation in the order written, hence no contraction. (Pb, Pd) leave as one 16-byte
// store for k_series_solar_gains; P goes into the step's row of `transmitted` where the caller takes one, and onto ap_sum.
// ANISO (heat_sky_aniso): the lane also loads its site's 16-byte coefficient pair and its band; the circumsolar part passes
// with the beam transmittance and the sunlit fraction. The instantiation without it is the kernel as it was.
template <bool ANISO>
__global__ void __launch_bounds__(256)
k_series_apertures(const SkyRecord *__restrict__ records, SeriesApertures ap, double *__restrict__ transmitted,
                   const SkyCoef *__restrict__ coef, const double *__restrict__ band) {
#pragma clang fp contract(off)
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = ap.n;
    if (a >= ap.n) return;
    const int d = ap.dev[a];
    const int site = ap.site ? ap.site[d] : 0;
    const SkyRecord r = records[site];
    const double nx = ap.normal[a], ny = ap.normal[n + a], nz = ap.normal[2 * n + a];
    const double c = (nx * r.sun_x + ny * r.sun_y) + nz * r.sun_z;
    const double fs = 0.5 + 0.5 * nz, fg = 0.5 - 0.5 * nz;
    double t = ap.coef[5 * n + a];
#pragma unroll
    for (int j = 4; j >= 0; j--) {
        t = t * c;
        t = t + ap.coef[j * n + a];
    }
    const double tau_diffuse = ap.tau_scale[a], scale = ap.tau_scale[n + a];
    const double ib = r.beam * c;
    double pb = c > 0.0 ? (ib * t) * scale : 0.0;
    const int j = ap.shade != nullptr ? ap.shade[a] : -1;  // (a kernel argument: without shades the branch is wave-uniform)
    double id;
    if (ANISO) {
        const SkyCoef q = coef[site];
        const double rb = aniso_rb(c, r.sun_z);
        const double iso = 1.0 - q.circ;
        const double pbm = (ib * t) * scale;
        const double ics = (r.diffuse * q.circ) * rb;
        const double pcs = (ics * t) * scale;
        double ps = pbm + pcs;
        double dd = (r.diffuse * fs) * iso;
        const double hv = (r.diffuse * q.horiz) * band[a];
        dd = dd + hv;
        double gg = r.ground * fg;
        if (j >= 0) {  // heat_shades
            ps = ps * ap.sf.f[j];
            dd = dd * ap.sf.diffuse[j];
            gg = gg * ap.sf.ground[j];
        }
        pb = c > 0.0 ? ps : 0.0;
        id = dd + gg;
    } else if (j >= 0) {  // heat_shades
        pb = c > 0.0 ? pb * ap.sf.f[j] : 0.0;
        id = (r.diffuse * fs) * ap.sf.diffuse[j] + (r.ground * fg) * ap.sf.ground[j];
    } else {
        id = r.diffuse * fs + r.ground * fg;
    }
    const double pd = (id * tau_diffuse) * scale;
    const double p = pb + pd;
    ap.power[a] = make_double2(pb, pd);
    if (transmitted != nullptr) transmitted[a] = p;
    if (ap.sum != nullptr) ap.sum[a] = ap.sum[a] + p;
}

// k_series_solar_gains — what the inside faces receive from the windows in one step, behind k_series_apertures and before
// the body: one lane per receiver (a side that has entries), 64 consecutive receivers a slice of the sliced-ELL tables
// (plan.hpp, SolarGainTables). In row i of its slice a wavefront reads 64 neighbouring aperture numbers and 64 neighbouring
// 16-byte share pairs, and gathers (Pb, Pd) of those apertures with 16-byte loads; a lane's sum is its own sequential chain
// in the caller's order — the layout does not enter the bits. From the raw value on it is the tail of sky_side for the
// solar field, restated: the gain, the mirror, the shared clamp, the side's absorptance factor, an 8-byte store. The side's
// long-wave field belongs to whoever drives it and is not touched.
__global__ void __launch_bounds__(256)
k_series_solar_gains(int n_surf, SeriesGains g, const double *__restrict__ side_alpha, SideDyn *__restrict__ dyn, SlotArrays sl,
                     double *__restrict__ mirror) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= g.n_receivers) return;
    const int lane = r & 63;
    const int64_t off = g.slice_off[r >> 6], rows = (g.slice_off[(r >> 6) + 1] - off) >> 6;
    double v = 0.0;
    for (int64_t i = 0; i < rows; i++) {
        const int64_t at = off + i * 64 + lane;
        const int a = g.ap[at];
        if (a < 0) continue;  // padding
        const double2 sh = g.share[at], p = g.power[a];
        v = v + sh.x * p.x;
        v = v + sh.y * p.y;
    }
    const int64_t rec = g.rec[r];
    const int side = rec >= n_surf;
    const int d = (int)(rec - (int64_t)side * n_surf);
    const double *const gain = side ? g.gain[1] : g.gain[0];
    if (gain != nullptr) v = v * gain[d];
    if (mirror != nullptr) mirror[(side ? sl.solar_b : sl.solar_f)[d]] = v;
    dyn[rec].solar = (side ? clamp_solar_back(v) : clamp_solar_front(v)) * side_alpha[rec];
}

// k_series_emission — sigma T^4 of every distinct emitter side of the room radiation in one step (heat_room_radiation,
// include/heat_amd.h), behind k_series_solar_gains: one lane per emitter. A lane reads its face node from the T buffer —
// the one scattered read of the pair of kernels, done once per emitter instead of once per viewer — and stores E into the
// compact array k_series_room_radiation gathers from. Nothing on the step's head writes T: every emitter is read as it was
// at the start of the step. The header's rule, one rounded operation per line, hence no contraction.
__global__ void __launch_bounds__(256)
k_series_emission(SeriesRoomRadiation rr, const double *__restrict__ T) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rr.n_emitters) return;
    const double tk = T[rr.face[j]] + 273.15;
    const double t2 = tk * tk;
    const double t4 = t2 * t2;
    rr.emission[j] = kSigma * t4;
}

// k_series_room_radiation — the long-wave irradiance of every receiver of the room radiation in one step, behind
// k_series_emission and before the body: one lane per receiver. A lane walks its CSR range of the entries (plan.hpp,
// RoomRadiationTables) — the ranges of neighbouring receivers are neighbours — and gathers E of the emitter from the compact
// array, or the channel's value from the step's row; its sum is its own sequential chain in the caller's order. From the raw
// value on it is the tail of sky_side for the long-wave field, restated: the gain, the mirror, the shared conversion, one
// 8-byte store. The side's solar field belongs to whoever drives it and is not touched. Every output has one writer: no
// atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_room_radiation(int n_surf, SeriesRoomRadiation rr, const double *__restrict__ row, SideDyn *__restrict__ dyn, SlotArrays sl,
                        double *__restrict__ mirror, double *__restrict__ irradiance_row) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rr.n_receivers) return;
    const int end = rr.off[r + 1];
    double v = 0.0;
    for (int at = rr.off[r]; at < end; at++) {
        const int j = rr.src[at];
        const double x = rr.factor[at] * (j >= 0 ? rr.emission[j] : row[~j]);
        v = v + x;
    }
    const int64_t rec = rr.rec[r];
    const int side = rec >= n_surf;
    const int d = (int)(rec - (int64_t)side * n_surf);
    const double *const gain = side ? rr.gain[1] : rr.gain[0];
    if (gain != nullptr) v = v * gain[d];
    if (irradiance_row != nullptr) irradiance_row[r] = v;
    if (rr.sum != nullptr) rr.sum[r] = rr.sum[r] + v;
    if (mirror != nullptr) mirror[(side ? sl.ir_b : sl.ir_f)[d]] = v;
    dyn[rec].rad_t = ir_to_rad_temperature(v);
}

// k_series_ambient — the ambient temperature of every driven side in one step (heat_ambient_drive, include/heat_amd.h), and
// the body of heat_batch_set_ambient (chan == nullptr: lane i takes row[i]; no gain, offset or mix): one lane per side over
// structure-of-arrays tables in the caller's order (plan.hpp, AmbientTables). The header's rule, one rounded operation per
// line, hence no contraction. A lane writes the `ambient` field of its side's record and, for a front whose back is Ambient
// as well, the `forced` field of that back record (its t_front source, layout.hpp) — plain 8-byte stores; the check has made
// sure that every record is named once, so every field has one writer. Nothing on the step's head writes the zone
// temperatures: every zone is read as it was at the start of the step. No LDS, no atomics.
__global__ void __launch_bounds__(256)
k_series_ambient(SeriesAmbient a, const double *__restrict__ row, const double *__restrict__ zone_T, SideConst *__restrict__ sc,
                 double *__restrict__ ambient_row) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_sides) return;
    double v = row[a.chan != nullptr ? a.chan[i] : i];
    if (a.gain != nullptr) v = a.gain[i] * v;
    if (a.offset != nullptr) v = v + a.offset[i];
    if (a.mix_zone != nullptr) {
        const int z = a.mix_zone[i];
        if (z >= 0) {
            const double d = zone_T[z] - v;
            const double m = a.mix[i] * d;
            v = v + m;
        }
    }
    sc[a.rec[i]].ambient = v;
    const uint32_t peer = a.peer[i];
    if (peer != kNoAmbientPeer) sc[peer].forced = v;
    if (ambient_row != nullptr) ambient_row[i] = v;
    if (a.sum != nullptr) a.sum[i] = a.sum[i] + v;
}

// Report of a series (heat_series_report, include/heat_amd.h): on the step's tail, beside k_series_probe. Everything below
// is written without contraction: the statistics are DEFINED as one rounded operation per rule, and a group's bits are to
// follow from its tables alone.
__device__ __forceinline__ double series_value(int b, uint32_t i, const double *__restrict__ T, const SideOut *__restrict__ out,
                                               const double *__restrict__ zone_T) {
    const double *base = b == kProbeBufT ? T : (b == kProbeBufOut ? reinterpret_cast<const double *>(out) : zone_T);
    return base[i];
}

// One lane's share of a segment: entries first, first + STRIDE, ... below end, added in that order.
template <int STRIDE>
__device__ __forceinline__ double series_group_lane(const SeriesGroupsDev &g, uint32_t first, uint32_t end, const double *__restrict__ T,
                                                    const SideOut *__restrict__ out, const double *__restrict__ zone_T) {
    double acc = 0.0;
    if (g.weight != nullptr) {
#pragma unroll 4
        for (uint32_t e = first; e < end; e += STRIDE) {
            const double p = g.weight[e] * series_value(g.buf[e], g.idx[e], T, out, zone_T);
            acc = acc + p;
        }
    } else {
#pragma unroll 4
        for (uint32_t e = first; e < end; e += STRIDE) acc = acc + series_value(g.buf[e], g.idx[e], T, out, zone_T);
    }
    return acc;
}

// k_series_groups — the segmented weighted gather-sum: one wavefront per segment of a large group (wavefronts
// [0, n_wave)), one 16-lane row per small group (four to a wavefront behind them). A lane adds its entries of the segment
// — lane-strided, so that a wave instruction reads 64 (16) neighbouring table entries and, the entries being sorted into
// device order, neighbouring records — and the lanes' sums go through the fixed DPP trees of k_zones. Which lane adds
// which entry, and the tree, follow from the segment's bounds alone: the partial sum does not depend on the grid, on the
// other segments or on timing. One writer per partial sum; no atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_groups(SeriesGroupsDev g, const double *__restrict__ T, const SideOut *__restrict__ out, const double *__restrict__ zone_T) {
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);  // (wave-uniform)
    if (w < g.n_wave) {
        const uint32_t *seg = g.wave_seg + 3 * (size_t)w;
        const uint32_t e0 = seg[0], e1 = seg[1];
        const double total = wave_sum_f64(series_group_lane<kWave>(g, e0 + lane, e1, T, out, zone_T));
        if (lane == 0) g.part[seg[2]] = total;
        return;
    }
    const int r = (w - g.n_wave) * 4 + (lane >> 4);
    uint32_t e0 = 0, e1 = 0, p = 0;
    if (r < g.n_row) {
        const uint32_t *seg = g.row_seg + 3 * (size_t)r;
        e0 = seg[0], e1 = seg[1], p = seg[2];
    }
    const double total = row_sum_f64(series_group_lane<16>(g, e0 + (lane & 15), e1, T, out, zone_T));  // in the row's lane 15
    if ((lane & 15) == 15 && r < g.n_row) g.part[p] = total;
}

// k_series_stats — one lane per quantity: a probe's value read as k_series_probe reads it, a group's as its segments'
// partial sums added in segment order (written to the step's group_trace row where there is one); then the rules of the
// header on the accumulators the caller asked for. An extremum is stored only when it changes.
__global__ void __launch_bounds__(256)
k_series_stats(SeriesStatsDev s, const double *__restrict__ T, const SideOut *__restrict__ out, const double *__restrict__ zone_T,
               double *__restrict__ group_row, int64_t step) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= s.n_probes + s.n_groups) return;
    double v;
    if (q < s.n_probes) {
        v = series_value(s.buf[q], s.idx[q], T, out, zone_T);
    } else {
        const int64_t g = q - s.n_probes;
        const uint32_t p0 = s.part_off[g], p1 = s.part_off[g + 1];
        v = p0 < p1 ? s.part[p0] : 0.0;
        for (uint32_t p = p0 + 1; p < p1; p++) v = v + s.part[p];
        if (group_row != nullptr) group_row[g] = v;
    }
    if (s.q_min != nullptr && v < s.q_min[q]) {
        s.q_min[q] = v;
        if (s.q_step_min != nullptr) s.q_step_min[q] = step;
    }
    if (s.q_max != nullptr && v > s.q_max[q]) {
        s.q_max[q] = v;
        if (s.q_step_max != nullptr) s.q_step_max[q] = step;
    }
    if (s.q_sum != nullptr) s.q_sum[q] = s.q_sum[q] + v;
    if (s.q_lo != nullptr) {
        const double lo = s.q_lo[q];
        if (v < lo) {
            if (s.q_n_below != nullptr) s.q_n_below[q] += 1;
            if (s.q_deg_below != nullptr) s.q_deg_below[q] = s.q_deg_below[q] + (lo - v);
        }
    }
    if (s.q_hi != nullptr) {
        const double hi = s.q_hi[q];
        if (v > hi) {
            if (s.q_n_above != nullptr) s.q_n_above[q] += 1;
            if (s.q_deg_above != nullptr) s.q_deg_above[q] = s.q_deg_above[q] + (v - hi);
        }
    }
}

// k_series_th_stats — one lane per thermostat (caller's order), behind k_series_zone_loads: the step's mode and applied
// power against the mode before the step.
__global__ void __launch_bounds__(256)
k_series_th_stats(int n, SeriesThStatsDev t, const uint8_t *__restrict__ mode, const double *__restrict__ applied_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = mode[i];
    if (t.steps_heating != nullptr && m == 1) t.steps_heating[i] += 1;
    if (t.steps_cooling != nullptr && m == 2) t.steps_cooling[i] += 1;
    if (t.switches != nullptr) {
        if (m != t.prev[i]) t.switches[i] += 1;
        t.prev[i] = (uint8_t)m;
    }
    if (t.sum_heating != nullptr || t.sum_cooling != nullptr) {
        const double a = applied_row[i];
        if (t.sum_heating != nullptr && a > 0.0) t.sum_heating[i] = t.sum_heating[i] + a;
        if (t.sum_cooling != nullptr && a < 0.0) t.sum_cooling[i] = t.sum_cooling[i] + a;
    }
}

// k_series_air_paths — the air paths of one step (heat_air_paths, include/heat_amd.h), behind k_series_zone_loads /
// k_series_th_stats and before k_series_inputs: one lane per zone walks the paths whose TARGET it is (a CSR range of the list
// sorted by target, the caller's order kept inside a zone) and adds the open ones to the a0 / b0 of its own zone alone; a zone
// nothing flows into leaves after reading its offsets. A path reads the temperature of its source zone — any zone — as the
// step before left it: nothing on the step's head writes zone_T, so every source is the start of the step's whatever the
// order of the lanes. A path belongs to the lane of its target: its state byte, its element of the step's path_q row and
// its accumulators (all in the caller's order, through `orig`) have one writer, and the order of a zone's sum is the
// caller's — which one lane per path with atomic adds would not give. Which outputs exist is decided by nullable pointers
// in the kernel argument: wave-uniform branches, an array nobody takes is neither read nor written.
// Every product and sum is one rounded operation in the header's order, the air properties written out as in
// k_series_zone_loads (same expressions, same grouping): the host applying the rule between march calls reproduces the bits.
// A NaN a0 / b0 is reported as the zone's failure, as the zone loads report it.
// control_T is what a controlled path senses for e alone: zone_T itself (the same pointer: the same bits as ever), or the
// step's control temperatures where a comfort sensor controls a zone (heat_comfort). The air that moves is air: g, dT and q
// keep zone_T.
__global__ void __launch_bounds__(256)
k_series_air_paths(int n_zones, AirPathsDev ap, const double *__restrict__ row, const double *__restrict__ zone_T,
                   const double *__restrict__ control_T, double *__restrict__ a0, double *__restrict__ b0, double *__restrict__ q_row,
                   int *__restrict__ flags) {
#pragma clang fp contract(off)
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n_zones) return;
    const int p0 = ap.off[z], p1 = ap.off[z + 1];
    if (p0 == p1) return;
    double a = a0[z], b = b0[z];
    const bool clean = a == a && b == b;
    const double tt = zone_T[z];
    for (int i = p0; i < p1; i++) {
        const int orig = ap.orig[i], src = ap.source[i], oc = ap.open_chan[i];
        const double ts = src >= 0 ? zone_T[src] : row[ap.temp_chan[i]];
        bool open = true, switched = false;
        if (oc >= 0) {
            const double set = row[oc], d = ap.half_band[i], s = ap.sense[i];
            const int before = ap.state[orig];
            const double e = s * (control_T[z] - set);
            const double g = s * (tt - ts);
            int now = before;
            if (e > d && g > ap.min_delta[i]) now = 1;
            else if (before == 1 && (e < -d || g <= 0.0)) now = 0;
            switched = now != before;
            if (switched) ap.state[orig] = (uint8_t)now;
            open = now == 1;
        }
        double q = 0.0;
        if (open) {
            const double v = ap.volume_gain[i] * row[ap.volume_chan[i]];
            const double tk = ts + 273.15;
            const double rho = 101325. * 28.97 / (8314.46261815324 * tk);  // gas.rs:175-179
            const double cp = 1002.7370 + 1.2324e-2 * tk;                  // gas.rs:49,165-167
            const double m = (rho * v) * cp;
            const double mt = m * ts;
            a = a + mt;
            b = b + m;
            const double dt = ts - tt;
            q = m * dt;
        }
        if (q_row != nullptr) q_row[orig] = q;
        if (ap.sum_q != nullptr) ap.sum_q[orig] = ap.sum_q[orig] + q;
        if (ap.steps_open != nullptr && open) ap.steps_open[orig] += 1;
        if (ap.switches != nullptr && switched) ap.switches[orig] += 1;
    }
    a0[z] = a;
    b0[z] = b;
    if (clean && (a != a || b != b)) report_failure(flags, FLAG_NAN_ZONE, (unsigned int)z);
}

// k_series_comfort — the operative temperature of every sensor in one step (heat_comfort, include/heat_amd.h), behind the
// step's head and before k_series_zone_loads: one lane per SENSOR. A lane walks its CSR range of entries (sorted by sensor,
// the caller's order kept inside a sensor) and gathers each face node straight from T: a scattered 8-byte load per entry,
// over entries whose (face, weight) pairs neighbouring lanes read from neighbouring ranges. A face usually belongs to one
// sensor, so a compact emitter list as in k_series_emission would buy nothing. The sum is the lane's own sequential chain in
// the caller's order — which a reduction over lanes would not give. Nothing on the step's head writes T or zone_T: every
// temperature is what the step before left. The header's rule, every line one rounded operation in the order written, hence
// no contraction; a NaN makes every comparison false. A sensor is one lane: its element of `top`, of the two rows and of
// every accumulator has one writer. Which outputs exist is decided by nullable pointers in the kernel argument:
// wave-uniform branches, an array nobody takes is neither read nor written. No atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_comfort(SeriesComfort cf, const double *__restrict__ row, const double *__restrict__ T, const double *__restrict__ zone_T,
                 double *__restrict__ operative_row, double *__restrict__ mrt_row, int64_t step) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cf.n_sensors) return;
    const int j0 = cf.off[i], j1 = cf.off[i + 1];
    double r = 0.0;
    int j = j0;
    // eight entries at a time: the gathers of a batch are in flight together (a long sensor would otherwise wait out one
    // memory latency per entry); the products are the same rounded operations and the sum keeps the caller's order
    for (; j + 8 <= j1; j += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = cf.weight[j + u] * T[cf.face[j + u]];
#pragma unroll
        for (int u = 0; u < 8; u++) r = r + x[u];
    }
    for (; j < j1; j++) {
        const double x = cf.weight[j] * T[cf.face[j]];
        r = r + x;
    }
    const double a = cf.air_weight[i];
    const double xa = a * zone_T[cf.zone[i]];
    const double b = 1.0 - a;
    const double xr = b * r;
    const double top = xa + xr;
    cf.top[i] = top;
    if (mrt_row != nullptr) mrt_row[i] = r;
    if (operative_row != nullptr) operative_row[i] = top;
    const int oc = cf.occ_chan[i];
    if (!(oc < 0 || row[oc] > 0.0)) return;
    if (cf.n_occupied != nullptr) cf.n_occupied[i] = cf.n_occupied[i] + 1;
    if (cf.sum_operative != nullptr) cf.sum_operative[i] = cf.sum_operative[i] + top;
    if (cf.min_operative != nullptr && top < cf.min_operative[i]) {
        cf.min_operative[i] = top;
        if (cf.step_min != nullptr) cf.step_min[i] = step;
    }
    if (cf.max_operative != nullptr && top > cf.max_operative[i]) {
        cf.max_operative[i] = top;
        if (cf.step_max != nullptr) cf.step_max[i] = step;
    }
    const int lc = cf.lo_chan[i], hc = cf.hi_chan[i];
    if (lc >= 0) {
        const double lo = row[lc];
        if (top < lo) {
            if (cf.n_below != nullptr) cf.n_below[i] = cf.n_below[i] + 1;
            const double d = lo - top;
            if (cf.deg_below != nullptr) cf.deg_below[i] = cf.deg_below[i] + d;
        }
    }
    if (hc >= 0) {
        const double hi = row[hc];
        if (top > hi) {
            if (cf.n_above != nullptr) cf.n_above[i] = cf.n_above[i] + 1;
            const double d = top - hi;
            if (cf.deg_above != nullptr) cf.deg_above[i] = cf.deg_above[i] + d;
            if (cf.max_above != nullptr && d > cf.max_above[i]) {
                cf.max_above[i] = d;
                if (cf.step_max_above != nullptr) cf.step_max_above[i] = step;
            }
        }
    }
}

// k_series_control_T — the control temperature of every zone in one step (heat_comfort), behind k_series_comfort and only
// when a sensor controls a zone: one lane per zone copies the operative temperature of the zone's control sensor (a gather
// from the step's `top`), or the zone's own temperature where it has none. The thermostats, the air paths' e and the blinds
// of the step read this array in place of zone_T.
__global__ void __launch_bounds__(256)
k_series_control_T(int n_zones, const int32_t *__restrict__ ctl_sensor, const double *__restrict__ top, const double *__restrict__ zone_T,
                   double *__restrict__ control_T) {
#pragma clang fp contract(off)
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n_zones) return;
    const int i = ctl_sensor[z];
    control_T[z] = i >= 0 ? top[i] : zone_T[z];
}

// k_series_handler_units — the air handlers of one step (heat_air_handlers, include/heat_amd.h), behind k_series_air_paths and
// before k_series_handler_supply: one lane per UNIT. A lane walks its CSR range of branches (sorted by unit, the caller's
// order kept inside a unit) twice, each a sequential chain of its own: the extract branches for the flow-weighted mix Te — a
// gather of zone temperatures nothing on the step's head writes: every one is the start of the step's —, then, with the
// bypass decided and the air properties taken behind the exchanger, the supply branches for their m[j] and the sum M. A
// reduction over lanes would not give the caller's order. The header's rule, every line one rounded operation in the order
// written, hence no contraction; a NaN makes every comparison false. Ts[u] and m[j] go to the call's scratch for
// k_series_handler_supply (m in the caller's branch order, through `orig`). A unit is one lane: its element of the three
// rows, its state byte and every accumulator have one writer; so has the branch_q of an extract-only branch, 0.0, which no
// zone's lane visits. Which outputs exist is decided by nullable pointers in the kernel argument: wave-uniform branches, an
// array nobody takes is neither read nor written. No atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_handler_units(HandlersDev h, const double *__restrict__ row, const double *__restrict__ zone_T, double *__restrict__ supply_row,
                       double *__restrict__ recovered_row, double *__restrict__ coil_row, double *__restrict__ branch_row) {
#pragma clang fp contract(off)
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= h.n_units) return;
    const int j0 = h.unit_off[u], j1 = h.unit_off[u + 1];
    const double to = row[h.outdoor_chan[u]];
    double st = 0.0, sv = 0.0;
    for (int j = j0; j < j1; j++) {
        if (!(h.u_kind[j] & 2)) continue;
        const double v = h.u_gain[j] * row[h.u_chan[j]];
        const double x = v * zone_T[h.u_zone[j]];
        st = st + x;
        sv = sv + v;
    }
    const double te = sv > 0.0 ? st / sv : to;
    double eta = h.eff_gain[u];
    const int ec = h.eff_chan[u], bc = h.bypass_chan[u], hc = h.heat_chan[u], cc = h.cool_chan[u];
    if (ec >= 0) eta = eta * row[ec];
    if (eta < 0.0) eta = 0.0;
    if (eta > 1.0) eta = 1.0;
    const int before = h.bypass[u];
    int now = before;
    if (bc >= 0) {
        const double set = row[bc], d = h.half_band[u];
        const double e = te - set;
        const double g = te - to;
        if (e > d && g > h.min_delta[u]) now = 1;
        else if (before == 1 && (e < -d || g <= 0.0)) now = 0;
        if (now != before) h.bypass[u] = (uint8_t)now;
        if (now == 1) eta = 0.0;
    }
    const double dt = te - to;
    const double r = eta * dt;
    const double tr = to + r;
    const double tk = tr + 273.15;
    const double rho = 101325. * 28.97 / (8314.46261815324 * tk);  // gas.rs:175-179
    const double cp = 1002.7370 + 1.2324e-2 * tk;                  // gas.rs:49,165-167
    double M = 0.0;
    for (int j = j0; j < j1; j++) {
        const int orig = h.u_orig[j];
        if (h.u_kind[j] & 1) {
            const double v = h.u_gain[j] * row[h.u_chan[j]];
            const double m = (rho * v) * cp;
            h.m[orig] = m;
            M = M + m;
        } else {  // (extracts only: nothing flows into its zone)
            if (branch_row != nullptr) branch_row[orig] = 0.0;
            if (h.sum_branch_q != nullptr) h.sum_branch_q[orig] = h.sum_branch_q[orig] + 0.0;
        }
    }
    const double recovered = M * r;
    double ts = tr, q = 0.0;
    bool heat_sat = false, cool_sat = false;
    const double heat_set = hc >= 0 ? row[hc] : 0.0, cool_set = cc >= 0 ? row[cc] : 0.0;
    if (hc >= 0 && tr < heat_set) {
        const double lift = heat_set - tr;
        const double need = M * lift;
        const double cap = h.heat_cap[u];
        if (need <= cap) {
            ts = heat_set;
            q = need;
        } else {
            q = cap;
            const double x = cap / M;
            ts = tr + x;
            heat_sat = true;
        }
    } else if (cc >= 0 && tr > cool_set) {
        const double drop = tr - cool_set;
        const double need = M * drop;
        const double cap = h.cool_cap[u];
        if (need <= cap) {
            ts = cool_set;
            q = 0.0 - need;
        } else {
            q = 0.0 - cap;
            const double x = cap / M;
            ts = tr - x;
            cool_sat = true;
        }
    }
    h.ts[u] = ts;
    if (supply_row != nullptr) supply_row[u] = ts;
    if (recovered_row != nullptr) recovered_row[u] = recovered;
    if (coil_row != nullptr) coil_row[u] = q;
    if (h.sum_recovered != nullptr) h.sum_recovered[u] = h.sum_recovered[u] + recovered;
    if (h.sum_heating != nullptr && q > 0.0) h.sum_heating[u] = h.sum_heating[u] + q;
    if (h.sum_cooling != nullptr && q < 0.0) h.sum_cooling[u] = h.sum_cooling[u] + q;
    if (h.steps_bypass != nullptr) h.steps_bypass[u] += now;
    if (h.switches != nullptr && now != before) h.switches[u] += 1;
    if (h.steps_heat_saturated != nullptr && heat_sat) h.steps_heat_saturated[u] += 1;
    if (h.steps_cool_saturated != nullptr && cool_sat) h.steps_cool_saturated[u] += 1;
}

// k_series_handler_supply — what the air handlers supply in one step, behind k_series_handler_units: one lane per ZONE walks
// the supply branches into it (a CSR range of the supply branches sorted by zone, the caller's order kept inside a zone) and
// adds m[j] * Ts[unit] and m[j] to the a0 / b0 of its own zone alone, behind what the zone loads and the air paths added; a
// zone without a branch leaves after reading its offsets. Ts and m are the scratch the units' kernel wrote in this step. A
// supply branch belongs to the lane of its zone: its element of the step's branch_q row and of sum_branch_q (the caller's
// order, through `orig`) has one writer. A NaN a0 / b0 is reported as the zone's failure, as the air paths report it.
__global__ void __launch_bounds__(256)
k_series_handler_supply(int n_zones, HandlersDev h, const double *__restrict__ zone_T, double *__restrict__ a0, double *__restrict__ b0,
                        double *__restrict__ branch_row, int *__restrict__ flags) {
#pragma clang fp contract(off)
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n_zones) return;
    const int p0 = h.zone_off[z], p1 = h.zone_off[z + 1];
    if (p0 == p1) return;
    double a = a0[z], b = b0[z];
    const bool clean = a == a && b == b;
    const double tz = zone_T[z];
    for (int i = p0; i < p1; i++) {
        const int orig = h.z_orig[i];
        const double m = h.m[orig], ts = h.ts[h.z_unit[i]];
        const double mt = m * ts;
        a = a + mt;
        b = b + m;
        const double dz = ts - tz;
        const double bq = m * dz;
        if (branch_row != nullptr) branch_row[orig] = bq;
        if (h.sum_branch_q != nullptr) h.sum_branch_q[orig] = h.sum_branch_q[orig] + bq;
    }
    a0[z] = a;
    b0[z] = b;
    if (clean && (a != a || b != b)) report_failure(flags, FLAG_NAN_ZONE, (unsigned int)z);
}

// k_series_vents — the demand vents of one step (heat_air_species, include/heat_amd.h), behind k_series_handler_supply and
// before k_series_species: one lane per ZONE walks its vents (a CSR range of the vents sorted by zone, the caller's order kept
// inside a zone), forms each one's volume flow from the concentration of the vent's species in this zone as the step starts
// with it — `conc` is not written in a step — and adds the enabled ones to the a0 / b0 of its own zone alone, behind what the
// loads, the paths and the handlers added; a zone without a vent leaves after reading its offsets. The header's rule, every
// line one rounded operation in the order written, the air properties written out as in k_series_zone_loads (same
// expressions, same grouping), hence no contraction; a NaN makes every comparison false. V goes to the call's scratch for
// k_series_species (the caller's order, through `orig`). A vent belongs to the lane of its zone: its elements of the two rows
// and of the three accumulators have one writer. Which outputs exist is decided by nullable pointers in the kernel argument:
// wave-uniform branches, an array nobody takes is neither read nor written. A NaN a0 / b0 is reported as the zone's failure,
// as the air paths report it. No atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_vents(int n_zones, SpeciesDev sp, const double *__restrict__ row, const double *__restrict__ zone_T,
               const double *__restrict__ conc, double *__restrict__ a0, double *__restrict__ b0, double *__restrict__ v_row,
               double *__restrict__ q_row, int *__restrict__ flags) {
#pragma clang fp contract(off)
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n_zones) return;
    const int p0 = sp.vent_off[z], p1 = sp.vent_off[z + 1];
    if (p0 == p1) return;
    double a = a0[z], b = b0[z];
    const bool clean = a == a && b == b;
    const double tz = zone_T[z];
    for (int i = p0; i < p1; i++) {
        const int orig = sp.v_orig[i], ec = sp.v_enable_chan[i];
        const double c = conc[(size_t)sp.v_species[i] * (size_t)n_zones + (size_t)z];
        const double lo = sp.c_lo[i], vmin = sp.v_min[i];
        const double x = c - lo;
        const double span = sp.c_hi[i] - lo;
        double f = x / span;
        if (f < 0.0) f = 0.0;
        if (f > 1.0) f = 1.0;
        bool saturated = f == 1.0;
        const double dv = sp.v_max[i] - vmin;
        const double y = f * dv;
        double V = vmin + y, q = 0.0;
        if (ec >= 0 && !(row[ec] > 0.0)) {
            V = 0.0;
            saturated = false;
        } else {
            const double t_in = row[sp.v_temp_chan[i]];
            const double tk = t_in + 273.15;
            const double rho = 101325. * 28.97 / (8314.46261815324 * tk);  // gas.rs:175-179
            const double cp = 1002.7370 + 1.2324e-2 * tk;                  // gas.rs:49,165-167
            const double m = (rho * V) * cp;
            const double mt = m * t_in;
            a = a + mt;
            b = b + m;
            const double dt = t_in - tz;
            q = m * dt;
        }
        sp.vent_V[orig] = V;
        if (v_row != nullptr) v_row[orig] = V;
        if (q_row != nullptr) q_row[orig] = q;
        if (sp.sum_volume != nullptr) sp.sum_volume[orig] = sp.sum_volume[orig] + V;
        if (sp.sum_q != nullptr) sp.sum_q[orig] = sp.sum_q[orig] + q;
        if (sp.steps_saturated != nullptr && saturated) sp.steps_saturated[orig] += 1;
    }
    a0[z] = a;
    b0[z] = b;
    if (clean && (a != a || b != b)) report_failure(flags, FLAG_NAN_ZONE, (unsigned int)z);
}

// What a lane of k_series_species reads of the other terms' tables: the zone loads' flows (ZoneLoadsDev), the air paths
// (AirPathsDev) and the handlers' supply branches by zone (HandlersDev) — the pointers of those views, nullptr offsets where
// the term is absent.
struct SpeciesInflows {
    const int32_t *fl_off, *fl_chan;               // [n_zones + 1], [n_flows] by zone
    const double *fl_gain;
    const int32_t *ap_off, *ap_source, *ap_chan, *ap_open_chan, *ap_orig;   // [n_zones + 1], [n_paths] by target
    const double *ap_gain;
    const uint8_t *ap_state;                       // [n_paths], the caller's order
    const int32_t *br_off, *br_orig;               // [n_zones + 1], [n_supply] by zone
};

// k_series_species — the concentrations of one step (heat_air_species, include/heat_amd.h), behind k_series_vents: one lane
// per (SPECIES, ZONE), lane = s * n_zones + z, so a wavefront reads neighbouring zones of one species: conc, the volumes, the
// offsets and the rows are plain coalesced loads. A lane sums its sources (a CSR range of the sources sorted by lane) and then
// every inflow into its zone in the header's order — the loads' flows, the air paths that are open behind this step's
// k_series_air_paths (the state bytes it has just written), the handlers' supply branches, the vents' V of this step's scratch
// — each a sequential chain in the caller's order, read through the tables those terms uploaded for their own kernels. A path
// from another zone gathers that zone's concentration out of `conc`, which no lane writes: every neighbour is the start of
// the step's, whatever the order of the lanes; the new value goes to conc_next, and the driver swaps the two between the
// steps. The header's rule, every line one rounded operation in the order written, hence no contraction; a NaN makes every
// comparison false. A lane's elements of the row and of the six accumulators have one writer. No atomics, no LDS.
__global__ void __launch_bounds__(256)
k_series_species(int n_zones, SpeciesDev sp, SpeciesInflows in, const double *__restrict__ row, const double *__restrict__ zone_vol,
                 double h, const double *__restrict__ conc, double *__restrict__ conc_next, double *__restrict__ conc_row, int64_t step) {
#pragma clang fp contract(off)
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= sp.n_species * n_zones) return;
    const int s = lane / n_zones, z = lane - s * n_zones;
    const double *const cs = conc + (size_t)s * (size_t)n_zones;
    const double c = cs[z], vol = zone_vol[z];
    const int oc = sp.outdoor_chan[lane];
    const double co = oc >= 0 ? row[oc] : 0.0;
    double S = 0.0, F = 0.0, G = 0.0;
    for (int i = sp.src_off[lane], i1 = sp.src_off[lane + 1]; i < i1; i++) {
        const double x = sp.src_factor[i] * row[sp.src_chan[i]];
        S = S + x;
    }
    if (in.fl_off != nullptr)
        for (int i = in.fl_off[z], i1 = in.fl_off[z + 1]; i < i1; i++) {
            const double V = in.fl_gain[i] * row[in.fl_chan[i]];
            const double g = V * co;
            F = F + V;
            G = G + g;
        }
    if (in.ap_off != nullptr)
        for (int i = in.ap_off[z], i1 = in.ap_off[z + 1]; i < i1; i++) {
            if (in.ap_open_chan[i] >= 0 && in.ap_state[in.ap_orig[i]] != 1) continue;
            const int src = in.ap_source[i];
            const double ci = src >= 0 ? cs[src] : co;
            const double V = in.ap_gain[i] * row[in.ap_chan[i]];
            const double g = V * ci;
            F = F + V;
            G = G + g;
        }
    if (in.br_off != nullptr)
        for (int i = in.br_off[z], i1 = in.br_off[z + 1]; i < i1; i++) {
            const int orig = in.br_orig[i];
            const double V = sp.br_gain[orig] * row[sp.br_chan[orig]];
            const double g = V * co;
            F = F + V;
            G = G + g;
        }
    if (sp.vent_off != nullptr)
        for (int i = sp.vent_off[z], i1 = sp.vent_off[z + 1]; i < i1; i++) {
            const double V = sp.vent_V[sp.v_orig[i]];
            const double g = V * co;
            F = F + V;
            G = G + g;
        }
    const double p = S + G;
    const double hp = h * p;
    const double vc = vol * c;
    const double num = vc + hp;
    const double hF = h * F;
    const double den = vol + hF;
    conc_next[lane] = num / den;
    if (conc_row != nullptr) conc_row[lane] = c;
    const int occ = sp.occ_chan[z];
    if (occ >= 0 && !(row[occ] > 0.0)) return;
    if (sp.n_occupied != nullptr) sp.n_occupied[lane] += 1;
    if (sp.sum_conc != nullptr) sp.sum_conc[lane] = sp.sum_conc[lane] + c;
    if (sp.max_conc != nullptr && c > sp.max_conc[lane]) {
        sp.max_conc[lane] = c;
        if (sp.step_max != nullptr) sp.step_max[lane] = step;
    }
    const int lc = sp.limit_chan[s];
    if (lc < 0) return;
    const double limit = row[lc];
    if (!(c > limit)) return;
    if (sp.n_above != nullptr) sp.n_above[lane] += 1;
    if (sp.excess_above != nullptr) sp.excess_above[lane] = sp.excess_above[lane] + (c - limit);
}

// sqrt, correctly rounded: the one rounded operation of the openings' rule that is not an add, a multiply or a divide, and the
// only sqrt of the series layer. It may be relied on because of how f64 sqrt lowers for gfx950 at the project's flags (-O3, no
// fast-math): v_rsq_f64 as the seed, a Goldschmidt refinement of s ~ sqrt(x) and h ~ 1 / (2 sqrt(x)), then two residual
// corrections d = fma(-s, s, x), s = fma(d, h, s) — the residual is exact in the fma, which is what lets the last step round
// correctly — with small inputs (subnormals among them) scaled up by v_ldexp_f64 first and the result scaled back, and 0 and
// +inf passed through by a class test. tests/test_openings_gpu.py holds it to numpy.sqrt bit for bit over squares and their
// neighbours, 4^n and 2 4^n +- 1 ulp, subnormals and both ends of the range. Named, so that a compiler whose lowering differs
// shows up in one place. (Here and not in device_math.hpp: the march does not call it.)
__device__ __forceinline__ double sqrt_rn(double x) { return sqrt(x); }

// k_series_openings — the openings of one step (heat_openings, include/heat_amd.h), first behind the controllers: one lane per
// opening over structure-of-arrays tables in the caller's order (plan.hpp, OpeningTables). A lane gathers its two
// temperatures from zone_T — which nothing on the step's head writes: every zone is read as it was at the start of the step
// — or one of them from the row, up to two more values from the row, forms V by the header's rule, every line one rounded
// operation in the order written, hence no contraction, and stores V into the row at its DERIVED channel: a plain 8-byte
// store. The check has made sure that no two openings share an out_chan and that no out_chan is a channel any opening reads,
// so every element of the row has one writer and no lane reads what another writes, whatever the order of the lanes; the
// kernels that read the derived columns are launched behind this one on the same stream. The absent outputs are
// wave-uniform branches. No LDS, no atomics, no scratch.
__global__ void __launch_bounds__(256)
k_series_openings(OpeningsDev op, double *row, const double *__restrict__ zone_T, double *__restrict__ v_row, int64_t step) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= op.n_openings) return;
    const int zb = op.zone_b[i];
    const double Ta = zone_T[op.zone_a[i]];
    const double Tb = zb >= 0 ? zone_T[zb] : row[op.temp_chan[i]];
    const double d = Ta - Tb;
    const double ad = fabs(d);
    const double sm = Ta + Tb;
    const double tm = sm * 0.5;
    const double tk = tm + 273.15;
    const double r = ad / tk;
    const double st = op.cs[i] * r;
    const double sa = op.ca[i] * ad;
    const int wc = op.wind_chan[i];
    const double u = wc >= 0 ? row[wc] : 0.0;
    const double u2 = u * u;
    const double w = op.cw[i] * u2;
    const double x = w + st;
    const double x2 = x + sa;
    double y = x2 + op.c0[i];
    if (y < 0.0) y = 0.0;
    const double U = sqrt_rn(y);
    const int fc = op.frac_chan[i];
    double f = fc >= 0 ? row[fc] : 1.0;
    if (f < 0.0) f = 0.0;
    if (f > 1.0) f = 1.0;
    const double af = op.area[i] * f;
    const double V = af * U;
    row[op.out_chan[i]] = V;
    if (v_row != nullptr) v_row[i] = V;
    if (op.sum_v != nullptr) op.sum_v[i] = op.sum_v[i] + V;
    if (op.max_v != nullptr && V > op.max_v[i]) {
        op.max_v[i] = V;
        if (op.step_max != nullptr) op.step_max[i] = step;
    }
}

// what a controller senses or limits on: a zone's air, a node of a wall, or a channel of the step's row
__device__ __forceinline__ double controller_reads(int kind, uint32_t at, const double *row, const double *__restrict__ T,
                                                   const double *__restrict__ zone_T) {
    return kind == 0 ? zone_T[at] : kind == 1 ? T[at] : row[at];
}

// k_series_controllers — the controllers of one step (heat_controllers, include/heat_amd.h), the FIRST kernel of the step,
// ahead of k_series_openings: one lane per controller over structure-of-arrays tables in the caller's order (plan.hpp,
// ControllerTables). A lane gathers what it senses and what limits it from zone_T and T — which nothing on the step's head
// writes: every temperature is read as it was at the start of the step — or from the row, its setpoint and its enable from
// the row, forms u and out by the header's rule, every line one rounded operation in the order written, hence no
// contraction, and stores out into the row at its DERIVED channel: a plain 8-byte store. The check has made sure that no two
// writers of the row (controllers and openings) share an out_chan and that no out_chan is a channel any controller reads, so
// every element of the row has one writer and no lane reads what another writes, whatever the order of the lanes; the
// openings and every consumer are launched behind this kernel on the same stream. The state (integral, tripped) is the
// lane's own element of its arrays. The absent outputs are wave-uniform branches. No LDS, no atomics, no scratch.
__global__ void __launch_bounds__(256)
k_series_controllers(ControllersDev ct, double *row, const double *__restrict__ T, const double *__restrict__ zone_T, double *__restrict__ u_row,
                     double *__restrict__ out_row) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ct.n_controllers) return;
    const double Ts = controller_reads(ct.sense_kind[i], ct.sense_at[i], row, T, zone_T);
    const double sp = row[ct.set_chan[i]];
    const double e0 = sp - Ts;
    const double e = ct.action[i] > 0 ? e0 : -e0;
    const int ec = ct.en_chan[i];
    const bool enabled = ec < 0 || row[ec] > 0.0;
    int trip = ct.tripped[i];
    const int lk = ct.lim_kind[i];
    if (lk >= 0) {
        const double Tl = controller_reads(lk, ct.lim_at[i], row, T, zone_T);
        if (Tl > ct.lim_hi[i]) {
            if (trip == 0 && ct.trips != nullptr) ct.trips[i] = ct.trips[i] + 1;
            trip = 1;
        } else if (trip == 1 && Tl < ct.lim_lo[i]) {
            trip = 0;
        }
        ct.tripped[i] = (uint8_t)trip;
    }
    double u;
    if (!enabled) {
        ct.integral[i] = 0.0;
        u = 0.0;
    } else if (trip == 1) {
        u = 0.0;
    } else {
        const double p = ct.kp[i] * e;
        const double ie = ct.ki[i] * e;
        double I1 = ct.integral[i] + ie;
        if (I1 < 0.0) I1 = 0.0;
        if (I1 > 1.0) I1 = 1.0;
        ct.integral[i] = I1;
        const double ub = p + I1;
        u = ub + ct.bias[i];
        if (u < 0.0) u = 0.0;
        if (u > 1.0) u = 1.0;
    }
    const double lo = ct.out_lo[i];
    const double span = ct.out_hi[i] - lo;
    const double o = u * span;
    const double out = lo + o;
    row[ct.out_chan[i]] = out;
    if (u_row != nullptr) u_row[i] = u;
    if (out_row != nullptr) out_row[i] = out;
    if (ct.sum_u != nullptr) ct.sum_u[i] = ct.sum_u[i] + u;
    if (ct.sum_out != nullptr) ct.sum_out[i] = ct.sum_out[i] + out;
    if (ct.steps_on != nullptr && u > 0.0) ct.steps_on[i] = ct.steps_on[i] + 1;
    if (ct.steps_sat != nullptr && u >= 1.0) ct.steps_sat[i] = ct.steps_sat[i] + 1;
}

// the density of dry air at t C: the expression and grouping of the air paths' rho
__device__ __forceinline__ double network_rho(double t) {
#pragma clang fp contract(off)
    const double tk = t + 273.15;
    return 101325. * 28.97 / (8314.46261815324 * tk);  // gas.rs:175-179
}

// One link of an air network by the header's rule, every line one rounded operation: q its volume flow, gm and ms what it adds
// to the diagonal and to the balance of its nodes. P: the pressures of the link's network (LDS), indexed by local node number.
struct NetworkLink {
    double q, gm, ms;
    bool fwd;
};
__device__ __forceinline__ NetworkLink network_link(const NetworksDev &nw, int l, const double *row, const double *__restrict__ zone_T,
                                                    const double *P) {
#pragma clang fp contract(off)
    const int fc = nw.frac_chan[l];
    double f = fc >= 0 ? row[fc] : 1.0;
    if (f < 0.0) f = 0.0;
    if (f > 1.0) f = 1.0;
    const double C = nw.c[l] * f;
    const int zb = nw.zone_b[l], lb = nw.lb[l];
    const double ra = network_rho(zone_T[nw.zone_a[l]]);
    const double rb = network_rho(zb >= 0 ? zone_T[zb] : row[nw.temp_chan[l]]);
    double pb = 0.0;
    if (lb >= 0) {
        pb = P[lb];
    } else {
        const int wc = nw.wp_chan[l];
        if (wc >= 0) pb = nw.wp_gain[l] * row[wc];
    }
    const double dr = ra - rb;
    const double sh = nw.gh[l] * dr;
    const double d0 = P[nw.la[l]] - pb;
    const double dp = d0 - sh;
    const double ad = fabs(dp);
    double q, gq;
    if (ad >= nw.p_lin[l]) {
        const double s = sqrt_rn(ad);
        q = C * s;
        const double hq = 0.5 * q;
        gq = hq / ad;
    } else {
        const double s_lin = nw.s_lin[l];
        const double ca = C * ad;
        q = ca / s_lin;
        gq = C / s_lin;
    }
    NetworkLink k;
    k.fwd = dp >= 0.0;
    const double ru = k.fwd ? ra : rb;
    const double m = ru * q;
    k.q = q;
    k.gm = ru * gq;
    k.ms = k.fwd ? m : -m;
    return k;
}

// k_series_networks<W> — the air networks of one width class for one step (heat_air_networks, include/heat_amd.h), launched
// behind the openings: a small nonlinear solve per network, not one lane per item. W lanes per network (its node count is at
// most W), a workgroup of ONE wavefront holding 64 / W networks (the last workgroup of a class is ragged), lane = node = row
// of A. The sorted tables are plan.hpp's NetworkTables; the outputs and the state go through net_id / node_id to the
// caller's order.
//   assemble: a lane walks its node's incident links in ascending link number and evaluates each itself — a zone-to-zone
//     link is evaluated by both of its lanes, with the same bits — adding into its own F and into its own row of A in LDS (a
//     runtime column index into a register array would go to scratch). Rows have the odd stride W + 1 doubles: the lanes of
//     a half-wave hit distinct banks on a column read, and the pivot row is a broadcast.
//   res: a cross-lane maximum over the network's W lanes, of |F| where that is > 0 and of 0 elsewhere: order-independent,
//     and a NaN never raises it, as in the rule.
//   eliminate: lane r updates row r against row kk; back-substitute by columns: each lane subtracts as d[j] appears.
// Every loop that encloses a barrier or a cross-lane operation has a wave-uniform bound: the largest n of the wavefront's
// networks, and "until every network of the wavefront has stopped" by __all, at most 65 assemblies since max_iter <= 64. A
// network that has stopped keeps walking with its writes masked. A lane of column i >= n of its network, or of a network past
// the class's end, walks too and touches nothing. The step's row is written at the links' derived columns only, by the lane
// of the link's first node: the check has made sure that they have one writer each and that no network reads them. No
// spin-wait, no atomics, no traffic between workgroups, no scratch.
template <int W>
__global__ void __launch_bounds__(64)
k_series_networks(NetworksDev nw, int first, int count, double *row, const double *__restrict__ zone_T, double *q_row, double *p_row,
                  int32_t *it_row) {
#pragma clang fp contract(off)
    constexpr int G = 64 / W, S = W + 1;
    __shared__ double A[64 * S];
    __shared__ double Fs[64], Ps[64], Ds[64];
    const int lane = threadIdx.x, g = lane / W, i = lane % W;
    const int in_class = blockIdx.x * G + g;
    const bool net_ok = in_class < count;
    const int s = first + (net_ok ? in_class : 0);
    const int n = net_ok ? nw.net_n[s] : 0;
    const bool mine = i < n;
    double *const An = A + g * W * S, *const Arow = An + i * S;
    double *const Fn = Fs + g * W, *const Pn = Ps + g * W, *const Dn = Ds + g * W;
    int nmax = n;
    for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, __shfl_xor(nmax, m));
    const double tol = net_ok ? nw.net_tol[s] : 0.0, g_min = net_ok ? nw.net_g_min[s] : 0.0;
    const int max_iter = net_ok ? nw.net_max_iter[s] : 0;
    int id = 0, inc0 = 0, inc_n = 0;
    double src = 0.0;
    Pn[i] = 0.0;
    if (mine) {
        const int p = nw.net_node0[s] + i;
        id = nw.node_id[p], inc0 = nw.node_inc0[p], inc_n = nw.node_inc_n[p];
        const int sc = nw.node_src_chan[p];
        if (sc >= 0) src = nw.node_src_gain[p] * row[sc];
        Pn[i] = nw.pressure[id];
    }
    double dold = 0.0, res = 0.0;
    bool done = !net_ok, conv = false;
    int iters = 0;
    __syncthreads();
    for (int it = 0; it <= 64; it++) {
        // ---- assemble ----
        double v = 0.0;
        if (mine && !done) {
            for (int j = 0; j < n; j++) Arow[j] = 0.0;
            double F = src, diag = g_min;
            for (int e = 0; e < inc_n; e++) {
                const int l = nw.inc[inc0 + e];
                const NetworkLink k = network_link(nw, l, row, zone_T, Pn);
                const int la = nw.la[l];
                if (la == i) {
                    F = F - k.ms;
                    const int lb = nw.lb[l];
                    if (lb >= 0) Arow[lb] = Arow[lb] - k.gm;
                } else {
                    F = F + k.ms;
                    Arow[la] = Arow[la] - k.gm;
                }
                diag = diag + k.gm;
            }
            Arow[i] = diag;
            Fn[i] = F;
            const double af = fabs(F);
            if (af > 0.0) v = af;
        }
        for (int m = W / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, W));
        if (!done) {
            res = v;
            if (it >= max_iter) {
                done = true, iters = it;
            } else if (res <= tol) {
                done = true, conv = true, iters = it;
            }
        }
        if (__all(done)) break;
        // ---- eliminate, no pivoting: lane r against row kk ----
        for (int kk = 0; kk < nmax - 1; kk++) {
            __syncthreads();
            if (mine && !done && i > kk) {
                const double *const Ak = An + kk * S;
                const double fac = Arow[kk] / Ak[kk];
                for (int j = kk + 1; j < n; j++) {
                    const double t = fac * Ak[j];
                    Arow[j] = Arow[j] - t;
                }
                const double t = fac * Fn[kk];
                Fn[i] = Fn[i] - t;
            }
        }
        // ---- back-substitute by columns ----
        double d = 0.0;
        for (int j = nmax - 1; j >= 0; j--) {
            if (mine && !done && i == j) {
                d = Fn[j] / Arow[j];
                Dn[j] = d;
            }
            __syncthreads();
            if (mine && !done && i < j && j < n) {
                const double t = Arow[j] * Dn[j];
                Fn[i] = Fn[i] - t;
            }
        }
        // ---- Walton's acceleration, per node ----
        if (mine && !done) {
            double w = 1.0;
            if (dold != 0.0) {
                const double r = d / dold;
                if (r < -0.5) {
                    const double o = 1.0 - r;
                    w = 1.0 / o;
                }
            }
            const double dn = w * d;
            Pn[i] = Pn[i] + dn;
            dold = dn;
        }
        __syncthreads();
    }
    // ---- write: the links by the lane of their first node, from the final pressures (those of the last assembly) ----
    if (!mine) return;
    const double Pi = Pn[i];
    nw.pressure[id] = Pi;
    if (p_row != nullptr) p_row[id] = Pi;
    for (int e = 0; e < inc_n; e++) {
        const int l = nw.inc[inc0 + e];
        if (nw.la[l] != i) continue;
        const NetworkLink k = network_link(nw, l, row, zone_T, Pn);
        const double ab = k.fwd ? k.q : 0.0, ba = k.fwd ? 0.0 : k.q;
        const int oab = nw.out_ab[l], oba = nw.out_ba[l];
        if (oab >= 0) row[oab] = ab;
        if (oba >= 0) row[oba] = ba;
        if (q_row != nullptr) q_row[l] = k.fwd ? k.q : -k.q;
        if (nw.sum_ab != nullptr) nw.sum_ab[l] = nw.sum_ab[l] + ab;
        if (nw.sum_ba != nullptr) nw.sum_ba[l] = nw.sum_ba[l] + ba;
    }
    if (i == 0) {
        const int w = nw.net_id[s];
        if (it_row != nullptr) it_row[w] = iters;
        if (nw.iters_sum != nullptr) nw.iters_sum[w] = nw.iters_sum[w] + iters;
        if (nw.unconverged != nullptr && !conv) nw.unconverged[w] = nw.unconverged[w] + 1;
        if (nw.max_res != nullptr && res > nw.max_res[w]) nw.max_res[w] = res;
    }
}

__global__ void __launch_bounds__(256) k_fill_f64(double *__restrict__ dst, int64_t n, double value) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = value;
}

// Ideal loads of a series (heat_ideal_loads, include/heat_amd.h): the zone update of a sub-timestep with the power that holds
// the setpoint. The rule is DEFINED as one rounded operation per line, in the header's order: no contraction here either.
// (The zone update itself, k_zone_update_ideal, is a zone kernel: kernels.hip, beside ideal_zone_rule.)
//
// k_series_ideal_begin — one lane per load, behind k_series_zone_loads: the step's setpoints out of the channel row (so
// that the sub-timestep kernel needs no per-step argument) and qsum = 0.
__global__ void __launch_bounds__(256) k_series_ideal_begin(IdealLoadsDev il, const double *__restrict__ row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= il.n_loads) return;
    const int hc = il.heat_chan[i], cc = il.cool_chan[i];
    il.setpoint[i] = hc >= 0 ? row[hc] : __builtin_nan("");
    il.setpoint[il.n_loads + i] = cc >= 0 ? row[cc] : __builtin_nan("");
    il.qsum[i] = 0.0;
}

// k_series_ideal_end — one lane per load, on the step's tail: the step's row of ideal_q and the accumulators that exist
// (the rules of k_series_stats with v = qsum). An extremum is stored only when it changes.
__global__ void __launch_bounds__(256) k_series_ideal_end(IdealLoadsDev il, double *__restrict__ q_row, int64_t step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= il.n_loads) return;
    const double v = il.qsum[i];
    if (q_row != nullptr) q_row[i] = v;
    if (il.sum_heating != nullptr && v > 0.0) il.sum_heating[i] = il.sum_heating[i] + v;
    if (il.sum_cooling != nullptr && v < 0.0) il.sum_cooling[i] = il.sum_cooling[i] + v;
    if (il.peak_heating != nullptr && v > il.peak_heating[i]) {
        il.peak_heating[i] = v;
        if (il.step_peak_heating != nullptr) il.step_peak_heating[i] = step;
    }
    if (il.peak_cooling != nullptr && v < il.peak_cooling[i]) {
        il.peak_cooling[i] = v;
        if (il.step_peak_cooling != nullptr) il.step_peak_cooling[i] = step;
    }
}
#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------
// Launch wrappers (host).
void launch_series_inputs(int n_surf, const double *row, const SeriesInputs &in, const double *T, const double *side_alpha,
                          SideDyn *dyn, const SlotArrays &sl, double *mirror, hipStream_t st) {
    if (n_surf <= 0) return;
    hipLaunchKernelGGL(k_series_inputs, dim3((n_surf + 255) / 256), dim3(256), 0, st, n_surf, row, in, T, side_alpha, dyn, sl, mirror);
}

void launch_series_sky(int n_surf, const SkyRecord *records, const SeriesSky &sky, const double *side_alpha, SideDyn *dyn,
                       const SlotArrays &sl, double *mirror, const SkyCoef *coef, const double *band, hipStream_t st) {
    if (n_surf <= 0) return;
    const dim3 grid((n_surf + 255) / 256);
    const double *no_band = nullptr;
    if (coef) hipLaunchKernelGGL(k_series_sky<true>, grid, dim3(256), 0, st, n_surf, records, sky, side_alpha, dyn, sl, mirror, coef, band);
    else hipLaunchKernelGGL(k_series_sky<false>, grid, dim3(256), 0, st, n_surf, records, sky, side_alpha, dyn, sl, mirror, coef, no_band);
}

void launch_series_shading(const SkyRecord *records, const SeriesShades &sh, double *sunlit_row, hipStream_t st) {
    if (sh.n <= 0) return;
    hipLaunchKernelGGL(k_series_shading, dim3((sh.n + 255) / 256), dim3(256), 0, st, records, sh, sunlit_row);
}

void launch_series_blinds(const SkyRecord *records, const SeriesBlinds &bl, const double *row, const double *zone_T,
                          double *position_row, double *incident_row, const SkyCoef *coef, const double *band, hipStream_t st) {
    if (bl.n_blinds <= 0 || bl.n_shades <= 0) return;
    const dim3 grid((bl.n_shades + 255) / 256);
    const double *no_band = nullptr;
    if (coef) hipLaunchKernelGGL(k_series_blinds<true>, grid, dim3(256), 0, st, records, bl, row, zone_T, position_row, incident_row, coef, band);
    else hipLaunchKernelGGL(k_series_blinds<false>, grid, dim3(256), 0, st, records, bl, row, zone_T, position_row, incident_row, coef, no_band);
}

void launch_series_apertures(const SkyRecord *records, const SeriesApertures &ap, double *transmitted, const SkyCoef *coef,
                             const double *band, hipStream_t st) {
    if (ap.n <= 0) return;
    const dim3 grid((ap.n + 255) / 256);
    const double *no_band = nullptr;
    if (coef) hipLaunchKernelGGL(k_series_apertures<true>, grid, dim3(256), 0, st, records, ap, transmitted, coef, band);
    else hipLaunchKernelGGL(k_series_apertures<false>, grid, dim3(256), 0, st, records, ap, transmitted, coef, no_band);
}

void launch_series_solar_gains(int n_surf, const SeriesGains &g, const double *side_alpha, SideDyn *dyn, const SlotArrays &sl,
                               double *mirror, hipStream_t st) {
    if (g.n_receivers <= 0) return;
    hipLaunchKernelGGL(k_series_solar_gains, dim3((g.n_receivers + 255) / 256), dim3(256), 0, st, n_surf, g, side_alpha, dyn, sl, mirror);
}

void launch_series_emission(const SeriesRoomRadiation &rr, const double *T, hipStream_t st) {
    if (rr.n_emitters <= 0) return;
    hipLaunchKernelGGL(k_series_emission, dim3((rr.n_emitters + 255) / 256), dim3(256), 0, st, rr, T);
}

void launch_series_room_radiation(int n_surf, const SeriesRoomRadiation &rr, const double *row, SideDyn *dyn, const SlotArrays &sl,
                                  double *mirror, double *irradiance_row, hipStream_t st) {
    if (rr.n_receivers <= 0) return;
    hipLaunchKernelGGL(k_series_room_radiation, dim3((rr.n_receivers + 255) / 256), dim3(256), 0, st, n_surf, rr, row, dyn, sl, mirror,
                       irradiance_row);
}

void launch_series_ambient(const SeriesAmbient &a, const double *row, const double *zone_T, SideConst *sc, double *ambient_row,
                           hipStream_t st) {
    if (a.n_sides <= 0) return;
    hipLaunchKernelGGL(k_series_ambient, dim3((a.n_sides + 255) / 256), dim3(256), 0, st, a, row, zone_T, sc, ambient_row);
}

void launch_series_zone_loads(int n_zones, const ZoneLoadsDev &zl, const double *row, const double *zone_T, double *a0, double *b0,
                              double *applied_row, int *flags, hipStream_t st) {
    if (n_zones <= 0) return;
    hipLaunchKernelGGL(k_series_zone_loads, dim3((n_zones + 255) / 256), dim3(256), 0, st, n_zones, zl, row, zone_T, a0, b0, applied_row,
                       flags);
}

void launch_series_probe(int64_t n_probes, const uint8_t *buf, const uint32_t *idx, const double *T, const SideOut *out,
                         const double *zone_T, double *trace_row, const int *flags, int *fail_step, int step, hipStream_t st) {
    // (at least one lane: lane 0 watches the failure flags also when nothing is probed)
    const int64_t n = std::max<int64_t>(n_probes, 1);
    hipLaunchKernelGGL(k_series_probe, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, st, n_probes, buf, idx, T, out, zone_T,
                       trace_row, flags, fail_step, step);
}

void launch_series_groups(const SeriesGroupsDev &g, const double *T, const SideOut *out, const double *zone_T, hipStream_t st) {
    const int n_waves = g.n_wave + (g.n_row + 3) / 4;
    if (n_waves <= 0) return;
    hipLaunchKernelGGL(k_series_groups, dim3(blocks_for_waves(n_waves)), dim3(256), 0, st, g, T, out, zone_T);
}

void launch_series_stats(const SeriesStatsDev &s, const double *T, const SideOut *out, const double *zone_T, double *group_row,
                         int64_t step, hipStream_t st) {
    const int64_t n = s.n_probes + s.n_groups;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_series_stats, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, st, s, T, out, zone_T, group_row, step);
}

void launch_series_th_stats(int n_thermostats, const SeriesThStatsDev &t, const uint8_t *mode, const double *applied_row, hipStream_t st) {
    if (n_thermostats <= 0) return;
    hipLaunchKernelGGL(k_series_th_stats, dim3((n_thermostats + 255) / 256), dim3(256), 0, st, n_thermostats, t, mode, applied_row);
}

void launch_series_air_paths(int n_zones, const AirPathsDev &ap, const double *row, const double *zone_T, const double *control_T,
                             double *a0, double *b0, double *q_row, int *flags, hipStream_t st) {
    if (n_zones <= 0) return;
    hipLaunchKernelGGL(k_series_air_paths, dim3((n_zones + 255) / 256), dim3(256), 0, st, n_zones, ap, row, zone_T, control_T, a0, b0, q_row,
                       flags);
}

void launch_series_comfort(const SeriesComfort &cf, const double *row, const double *T, const double *zone_T, double *operative_row,
                           double *mrt_row, int64_t step, hipStream_t st) {
    if (cf.n_sensors <= 0) return;
    hipLaunchKernelGGL(k_series_comfort, dim3((cf.n_sensors + 255) / 256), dim3(256), 0, st, cf, row, T, zone_T, operative_row, mrt_row, step);
}

void launch_series_control_T(int n_zones, const int32_t *ctl_sensor, const double *top, const double *zone_T, double *control_T,
                             hipStream_t st) {
    if (n_zones <= 0) return;
    hipLaunchKernelGGL(k_series_control_T, dim3((n_zones + 255) / 256), dim3(256), 0, st, n_zones, ctl_sensor, top, zone_T, control_T);
}

void launch_series_handler_units(const HandlersDev &h, const double *row, const double *zone_T, double *supply_row, double *recovered_row,
                                 double *coil_row, double *branch_row, hipStream_t st) {
    if (h.n_units <= 0) return;
    hipLaunchKernelGGL(k_series_handler_units, dim3((h.n_units + 255) / 256), dim3(256), 0, st, h, row, zone_T, supply_row, recovered_row,
                       coil_row, branch_row);
}

void launch_series_handler_supply(int n_zones, const HandlersDev &h, const double *zone_T, double *a0, double *b0, double *branch_row,
                                  int *flags, hipStream_t st) {
    if (n_zones <= 0 || h.n_units <= 0) return;
    hipLaunchKernelGGL(k_series_handler_supply, dim3((n_zones + 255) / 256), dim3(256), 0, st, n_zones, h, zone_T, a0, b0, branch_row, flags);
}

void launch_series_vents(int n_zones, const SpeciesDev &sp, const double *row, const double *zone_T, const double *conc, double *a0,
                         double *b0, double *v_row, double *q_row, int *flags, hipStream_t st) {
    if (n_zones <= 0 || sp.n_vents <= 0) return;
    hipLaunchKernelGGL(k_series_vents, dim3((n_zones + 255) / 256), dim3(256), 0, st, n_zones, sp, row, zone_T, conc, a0, b0, v_row, q_row,
                       flags);
}

void launch_series_species(int n_zones, const SpeciesDev &sp, const ZoneLoadsDev *zl, const AirPathsDev *ap, const HandlersDev *hd,
                           const double *row, const double *zone_vol, double h, const double *conc, double *conc_next, double *conc_row,
                           int64_t step, hipStream_t st) {
    const int64_t lanes = (int64_t)sp.n_species * n_zones;
    if (lanes <= 0) return;
    SpeciesInflows in{};
    if (zl) in.fl_off = zl->off + (n_zones + 1), in.fl_chan = zl->flow_volume_chan, in.fl_gain = zl->flow_volume_gain;
    if (ap)
        in.ap_off = ap->off, in.ap_source = ap->source, in.ap_chan = ap->volume_chan, in.ap_open_chan = ap->open_chan, in.ap_orig = ap->orig,
        in.ap_gain = ap->volume_gain, in.ap_state = ap->state;
    if (hd) in.br_off = hd->zone_off, in.br_orig = hd->z_orig;
    hipLaunchKernelGGL(k_series_species, dim3((unsigned int)((lanes + 255) / 256)), dim3(256), 0, st, n_zones, sp, in, row, zone_vol, h, conc,
                       conc_next, conc_row, step);
}

void launch_series_openings(const OpeningsDev &op, double *row, const double *zone_T, double *v_row, int64_t step, hipStream_t st) {
    if (op.n_openings <= 0) return;
    hipLaunchKernelGGL(k_series_openings, dim3((op.n_openings + 255) / 256), dim3(256), 0, st, op, row, zone_T, v_row, step);
}

void launch_series_controllers(const ControllersDev &ct, double *row, const double *T, const double *zone_T, double *u_row, double *out_row,
                               hipStream_t st) {
    if (ct.n_controllers <= 0) return;
    hipLaunchKernelGGL(k_series_controllers, dim3((ct.n_controllers + 255) / 256), dim3(256), 0, st, ct, row, T, zone_T, u_row, out_row);
}

template <int W>
static void launch_networks_class(const NetworksDev &nw, int c, double *row, const double *zone_T, double *q_row, double *p_row, int32_t *it_row,
                                  hipStream_t st) {
    constexpr int G = 64 / W;
    const int first = nw.class_start[c], count = nw.class_start[c + 1] - first;
    if (count <= 0) return;
    hipLaunchKernelGGL(k_series_networks<W>, dim3((count + G - 1) / G), dim3(64), 0, st, nw, first, count, row, zone_T, q_row, p_row, it_row);
}

void launch_series_networks(const NetworksDev &nw, double *row, const double *zone_T, double *q_row, double *p_row, int32_t *it_row,
                            hipStream_t st) {
    launch_networks_class<8>(nw, 0, row, zone_T, q_row, p_row, it_row, st);
    launch_networks_class<16>(nw, 1, row, zone_T, q_row, p_row, it_row, st);
    launch_networks_class<32>(nw, 2, row, zone_T, q_row, p_row, it_row, st);
    launch_networks_class<64>(nw, 3, row, zone_T, q_row, p_row, it_row, st);
}

void launch_fill_f64(double *dst, int64_t n, double value, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_fill_f64, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, st, dst, n, value);
}

void launch_series_ideal_begin(const IdealLoadsDev &il, const double *row, hipStream_t st) {
    if (il.n_loads <= 0) return;
    hipLaunchKernelGGL(k_series_ideal_begin, dim3((il.n_loads + 255) / 256), dim3(256), 0, st, il, row);
}

void launch_series_ideal_end(const IdealLoadsDev &il, double *q_row, int64_t step, hipStream_t st) {
    if (il.n_loads <= 0) return;
    hipLaunchKernelGGL(k_series_ideal_end, dim3((il.n_loads + 255) / 256), dim3(256), 0, st, il, q_row, step);
}

}  // namespace heat
