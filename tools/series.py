"""Series march (heat_batch_march_series) against the per-call path, on the headline model (1 M walls x 32 nodes, 10 000
zones): 64 channels, every surface driven on all four inputs, probes = all zones; n_sub = 2 and 20. Three legs, alternated
in one process, host clock around work that ends in a synchronisation:
  A  per-call drop-in: heat_batch_march_ex(SURFACE_SCALARS | ZONE_TEMPERATURES) per step, numpy writing the inputs into the
     caller's state between the calls (reported with and without the time numpy takes: a compiled host writes faster)
  B  march_resident alone, same n_sub, nothing driven, one synchronisation at the end: the floor
  C  march_series: one call for all steps, schedules uploaded inside the clock
Prints ms per step of each, C / A and C - B (also without the set-up of the call, from a series of one step), and writes profiles/series_march.json.
With --loads two other legs, alternated in the same way, one gain, one infiltration flow and one thermostat per zone
(heat_batch_march_series_loads):
  C  march_series carrying [steps][n_zones] rows of zone a0 / b0 the host computed in advance (the gains and flows; a
     thermostat cannot be a row at all) — what a series offered for these terms before the loads
  D  march_series with the loads formed on the device at every step
and writes profiles/series_loads.json: ms per step of each, D / C, and a series of one step of each.
With --report (heat_batch_march_series_report; the loads of --loads) four legs, alternated in the same way:
  D  march_series with the loads, probes = all zones (the leg of --loads, re-measured here)
  E  the same series tracing all zones and both convective flows of every wall, then numpy on the host: minimum, maximum, sum
     and steps above 26 C of every zone, one area-weighted envelope-flow sum per zone and step, the thermostats' steps, switches
     and sums from the applied rows — the only way to these numbers without a report
  F  the same series with a report and no trace: those statistics of every zone and of one envelope-flow group per zone, and
     the thermostat statistics
  G  F with the inside-face node of every wall as further probes (Q = S + 2 Z) and q_min alone; G4: with F's four statistics
and writes profiles/series_report.json.
With --ideal (heat_batch_march_series_ideal; the channels, driven inputs and loads of --loads plus a cooling setpoint channel) four
legs, alternated in the same way, one ideal load per zone, heating and cooling, unlimited:
  S  the series with leg D's loads on a batch created with no_fusion: the streamed body the ideal path is built on
  I  the same plus the ideal loads (same batch)
  R  leg I on the batch of leg D with heat_batch_set_ideal_resident: the ideal loads inside the cluster-resident march
     (the opt-in is switched off again for leg D, which must stay the plain resident series)
  D  leg D itself, on the batch as planned (cluster-resident)
and writes profiles/series_ideal.json: ms per step of each, I - S per sub-timestep, I / S, I / D, R / D and R / I.
With --sky (heat_batch_march_series_sky; the model, channels, loads and probes of leg D) two legs, alternated in the same way:
  C' every wall's front solar and front long-wave input driven from channels (64 columns shared by all walls: what a channel
     table can hold; with a column per wall — what walls of their own azimuth need — the table is 16 S bytes per step)
  K  the same two inputs of every wall formed on the device from the sky: every wall its own azimuth, one site, one 64-byte
     record per step, the sun from heat_amd.sky.sun_direction (day 172, latitude 48 N, the steps spread over the day)
and writes profiles/series_sky.json: ms per step of each, K / C', K - C'.
With --gains (heat_batch_march_series_gains; the model, channels, loads and probes of leg D; every tenth wall of a zone an
aperture, the zone-facing side of every other wall of the zone a receiver of all the zone's apertures: at 1 M walls 100 k
apertures, 900 k receivers, 9 M entries) two legs, alternated in the same way:
  H  what a series offered before: every receiver's back solar input driven from a channel column of its own, the host
     computing the columns (the rule of heat_amd/solar_gains.py over index arrays prepared once) and widening the table
     INSIDE the clock
  J  the same series with gains: one 64-byte sky record per step, the entry list given as it is
beside leg D (the same series without the receivers: their input from the shared channels like everybody's), and writes
profiles/series_gains.json: ms per step of each, J / H, a series of ONE step of each, J - D once the calls are set up, the
bytes a step of k_series_solar_gains and of leg J's k_series_inputs moves.
With --air (heat_batch_march_series_air; the model, channels, loads and probes of leg D; the zones taken ten to a building:
a doorway — two paths — between neighbouring zones of a building, 1.8 paths per zone, and one controlled outdoor vent per
zone, a cooling vent on the outdoor temperature channel) two legs, alternated in the same way:
  D  leg D itself: the series with loads and no paths
  A  the same series with the air paths
and writes profiles/series_air.json: ms per step of each, A - D, a series of ONE step of each, and — where the kernel trace of
one A series has been taken (--one-series --air under rocprofv3 --kernel-trace --stats, a run of its own) —
k_series_air_paths beside the same trace's k_series_zone_loads and whether A <= 1.05 (D + k_series_air_paths).
With --shades (heat_batch_march_series_shaded; the model, channels, loads, probes, records and normals of --sky) two legs,
alternated in the same way:
  K  the --sky leg K, run again in the same process;
  S  K with every wall's front solar input shaded by a shade of its own in the wall's plane: an overhang, two fins and the
     site's horizon profile
and writes profiles/series_shades.json: ms per step of each, S - K against the expectation
S - K <= 1.5 x (188 B per shade / 2.0 TB/s) (160 B of k_series_shading's own, 28 B gathered per shaded side in k_series_sky), a
series of ONE step of each, and — where the kernel trace of one S series has been taken (--one-series --shades under
rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_shades_kernel_stats.csv) — k_series_shading per step.
With --radiation (heat_batch_march_series_radiation; NOT the 100-wall zones of the headline: the same walls in rooms of 7
faces, 6-8 where the count does not divide — Z = S / 7 —, channels, loads and probes as in leg D; the back of every wall a
receiver that sees the backs of all walls of its room, itself included, by heat_amd.room_radiation.exchange_by_area: at 1 M
walls 1 M receivers, 1 M distinct emitters, 7 M entries) two legs, alternated in the same way:
  D  leg D on this model: every receiver's long-wave input driven from the 64 shared channels like everybody's
  R  the same series with the backs' long-wave input formed by the room radiation instead (irradiance not recorded)
and writes profiles/series_radiation.json: ms per step of each, R - D, a series of ONE step of each and the per-step times
once the calls are set up, the bytes a step of k_series_emission and k_series_room_radiation moves. No time is a pass
criterion.
With --ambient (heat_batch_march_series_ambient; the headline's walls with the back side of one wall in ten turned to
Boundary::AmbientTemperature — at 1 M walls 100 000 driven sides —, channels, loads and probes as in leg D plus four
temperature channels) two legs, alternated in the same way:
  N  the series with loads and the drive NULL: the launches of the parent's path
  M  the same series with every Ambient back driven from a temperature channel with a gain and an offset, every second one
     mixed (b = 0.5) with the temperature of the zone next to its wall's own (ambient_t not recorded)
and writes profiles/series_ambient.json: ms per step of each, M - N, a series of ONE step of each and the per-step times once
the calls are set up, the bytes a step of k_series_ambient moves, and — where the kernel trace of one M series has been taken
(--one-series --ambient under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_ambient_kernel_stats.csv) —
k_series_ambient per step. No time is a pass criterion.
With --blinds (heat_batch_march_series_blinds; the model, channels, loads, probes, records, normals and shades of --shades plus
three channels: a position schedule, an enable schedule and a cooling setpoint) two legs, alternated in the same way:
  S  the --shades leg S, run again in the same process with blinds = None: the launches of the parent's path
  B  S with a blind on every shade — in turn scheduled; controlled by the irradiance alone; gated by the temperature of the
     wall's zone; gated and with an enable schedule — (position and blind_incident not recorded)
and writes profiles/series_blinds.json: ms per step of each, B - S, a series of ONE step of each and the per-step times once
the calls are set up, the bytes a step of k_series_blinds moves, and — where the kernel trace of one B series has been taken
(--one-series --blinds under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_blinds_kernel_stats.csv) —
k_series_blinds per step beside the same trace's k_series_shading. No time is a pass criterion.
With --aniso (heat_batch_march_series_call with an anisotropic sky, heat_sky_aniso; everything of --blinds plus Reindl's
coefficients of the day's records and Reindl's band of every wall and shade) it alternates
  B  the --blinds leg B through the positional entry point, aniso = None: the isotropic kernels
  A  the same call with aniso given: the anisotropic instantiations of k_series_blinds and k_series_sky
and writes profiles/series_aniso.json: ms per step of each, A - B, a series of ONE step of each and the per-step times once the
calls are set up, and — where the kernel trace of one A series has been taken (--one-series --aniso under rocprofv3
--kernel-trace --stats, a run of its own; profiles/series_aniso_kernel_stats.csv) — the kernels' own times. No time is a pass
criterion.
With --comfort (heat_batch_march_series_comfort, heat_comfort; the loads of --loads, whose thermostats then sense) it alternates
  N  the series with loads through heat_batch_march_series_call, comfort = NULL
  C  the same call with one sensor per zone by comfort.by_area, every sensor the control temperature of its zone, occupancy
     and an adaptive band in three channels, every accumulator kept (operative and mrt not recorded)
and writes profiles/series_comfort.json: ms per step of each, C - N, a series of ONE step of each and the per-step times once
the calls are set up, the bytes a step of the two kernels moves, and — where the kernel trace of one C series has been taken
(--one-series --comfort under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_comfort_kernel_stats.csv) —
k_series_comfort and k_series_control_T per step. No time is a pass criterion.
With --handlers (heat_batch_march_series_handlers, heat_air_handlers; the loads of --loads) it alternates
  N  the series with loads through heat_batch_march_series_handlers, handlers = NULL
  H  the same call with one unit for every five zones: five balanced branches, a bypass, a heating and a cooling coil each
and writes profiles/series_handlers.json: ms per step of each, H - N, a series of ONE step of each (the call's set-up) and the
per-step times once the set-up is taken off — and, where a kernel trace of one H series has been taken (--one-series --handlers
under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_handlers_kernel_stats.csv), k_series_handler_units
and k_series_handler_supply per step. No time is a pass criterion.
With --species (heat_batch_march_series_species, heat_air_species; the loads and the handlers of --handlers) it alternates
  N  the series with loads and handlers through heat_batch_march_series_species, species = NULL
  P  the same call with two species, one demand vent and one source per zone, a limit and every accumulator kept
and writes profiles/series_species.json: ms per step of each, P - N, a series of ONE step of each (the call's set-up) and the
per-step times once the set-up is taken off — and, where a kernel trace of one P series has been taken (--one-series --species
under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_species_kernel_stats.csv), k_series_vents and
k_series_species per step. No time is a pass criterion.
With --openings (heat_batch_march_series_openings, heat_openings; the loads, handlers and species of --species, plus per zone one
opening to outside that feeds a CONTROLLED supply path — a night-ventilation window — and per pair of neighbouring zones one
doorway opening that feeds the two paths of air_paths.doorway) it alternates
  C  the series with openings = NULL and the SAME flows precomputed into ordinary channels: the opening_v rows of one O series,
     written into the columns the paths read (the march then computes the same bits: the tool asserts equal traces)
  O  the same call with the openings, the derived columns of the host table NaN
and writes profiles/series_openings.json: ms per step of each, O - C, a series of ONE step of each (the call's set-up) and the
per-step times once the set-up is taken off — and, where a kernel trace of one O series has been taken (--one-series --openings
under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_openings_kernel_stats.csv), k_series_openings per step.
No time is a pass criterion.
With --controllers (heat_batch_march_series_controllers, heat_controllers; the --openings workload, plus per zone one
proportional valve on the zone's air that feeds a gain of the zone loads and per opening one PI loop on its zone's air, cooling
action, that feeds the opening's open fraction) it alternates
  P  the series with controllers = NULL and the SAME outputs precomputed into ordinary channels: the control_out rows of one K
     series, written into the columns the gains and the openings read (the tool asserts equal traces)
  K  the same call with the controllers, the derived columns of the host table NaN
and writes profiles/series_controllers.json: ms per step of each, K - P, a series of ONE step of each (the call's set-up) and the
per-step times once the set-up is taken off — and, where a kernel trace of one K series has been taken (--one-series
--controllers under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_controllers_kernel_stats.csv),
k_series_controllers per step. No time is a pass criterion.
With --networks (heat_batch_march_series_networks, heat_air_networks; the --controllers workload, plus one air network per
building of ten zones: nine doorways, every other one a tall opening of two links, and one link to outside per zone at its
storey's height behind the wind pressure of one of two facades, every derived column read by an air path) it alternates
  F  the series with networks = NULL and the SAME flows fed back as ordinary channels: the link_q rows of one W series
     (equal traces asserted)
  W  the same call with the networks, the derived columns of the host table NaN
and writes profiles/series_networks.json: ms per step of each with their spreads, W - F, a series of ONE step of each (the
call's set-up), how many networks, nodes and links that is and, where a kernel trace of one W series has been taken
(--one-series --networks under rocprofv3 --kernel-trace --stats, a run of its own; profiles/series_networks_kernel_stats.csv),
k_series_networks per step and per width class. No time is a pass criterion.
  python tools/series.py [S] [steps] [rounds] [--out=FILE] [--loads | --report | --ideal | --sky | --gains | --air | --shades | --radiation | --ambient | --blinds | --aniso | --comfort | --handlers | --species | --openings | --controllers | --networks]
  python tools/series.py --one-series [S] [steps] [--loads | --report | --report=one-group | --report=nodes | --ideal | --sky | --gains | --air | --shades | --radiation | --ambient | --blinds | --comfort | --handlers | --species | --openings | --controllers | --networks]
                                                     one warm-up series and one more of n_sub = 2, nothing else (to run under
                                                     rocprofv3 --kernel-trace --stats): leg F; with one-group a single group
                                                     over the flows of all sides instead of one per zone; with nodes leg G;
                                                     with --ideal leg I; with --sky a series of leg C' and one of leg K; with --gains
                                                     a series of leg J; with --air a series of leg A; with --shades a series of leg S;
                                                     with --radiation a series of leg R; with --ambient a series of leg M; with --blinds a series
                                                     of leg B; with --comfort a series of leg C"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from heat_amd import HeatBatch, air_networks as anm, controllers as ctm, openings as opm, air_handlers as ahm, air_species as aspm, ambient as ambm, air_paths as apm, comfort as cfm, modeldict as mdl, room_radiation as rrm, shading as shm, sky as skym, solar_gains as sgm
ONE = "--one-series" in sys.argv
REPORT = next((a[9:] or "zones" for a in sys.argv[1:] if a == "--report" or a.startswith("--report=")), None)
IDEAL = "--ideal" in sys.argv
SKY = "--sky" in sys.argv
GAINS = "--gains" in sys.argv
AIR = "--air" in sys.argv
ANISO = "--aniso" in sys.argv
BLINDS = "--blinds" in sys.argv or ANISO
SHADES = "--shades" in sys.argv or BLINDS
RADIATION = "--radiation" in sys.argv
AMBIENT = "--ambient" in sys.argv
COMFORT = "--comfort" in sys.argv
NETWORKS = "--networks" in sys.argv
CONTROLLERS = "--controllers" in sys.argv or NETWORKS
OPENINGS = "--openings" in sys.argv or CONTROLLERS
SPECIES = "--species" in sys.argv or OPENINGS
HANDLERS = "--handlers" in sys.argv or SPECIES
LOADS = "--loads" in sys.argv or REPORT is not None or IDEAL or SKY or GAINS or AIR or SHADES or RADIATION or AMBIENT or COMFORT or HANDLERS
OUT = next((a[6:] for a in sys.argv[1:] if a.startswith("--out=")), None)
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(ARGS[0]) if len(ARGS) > 0 else 1_000_000
STEPS = int(ARGS[1]) if len(ARGS) > 1 else 100
ROUNDS = int(ARGS[2]) if len(ARGS) > 2 else 3
N_CHANNELS = 64
KEYS = ("solar_front", "solar_back", "ir_front", "ir_back")

md, st0 = mdl.uniform_massive(S, n=32, Z=max(1, S // (7 if RADIATION else 100)), dt=45.0)
rng = np.random.default_rng(1)
if AMBIENT:
    # the back of one wall in ten faces an ambient temperature (a ground slab, a neighbour, an unheated space)
    ambient_walls = np.arange(0, S, 10, dtype=np.int64)
    md["back_kind"] = np.where(np.arange(S) % 10 == 0, mdl.AMBIENT, md["back_kind"]).astype(np.int32)
    md["back_ambient"] = np.where(np.arange(S) % 10 == 0, 12.0, md["back_ambient"])
channel = np.concatenate([rng.uniform(0.0, 600.0, (STEPS, N_CHANNELS // 2)), rng.uniform(300.0, 450.0, (STEPS, N_CHANNELS // 2))], axis=1)
drives = {k: ((rng.integers(0, N_CHANNELS // 2, S) + (N_CHANNELS // 2 if i >= 2 else 0)).astype(np.int32), rng.uniform(0.5, 1.5, S))
          for i, k in enumerate(KEYS)}
probes = md["zone_slot"]
# --loads: four more channels (gain power W, infiltration m3/s, outdoor C, heating setpoint C) and one term of each kind per zone
Z = int(md["n_zones"])
if LOADS:
    channel = np.concatenate([channel, rng.uniform(0.0, 300.0, (STEPS, 1)), rng.uniform(0.0, 0.05, (STEPS, 1)),
                              rng.uniform(-5.0, 35.0, (STEPS, 1)), rng.uniform(19.0, 21.0, (STEPS, 1))], axis=1)
    every, full = np.arange(Z, dtype=np.int32), lambda c: np.full(Z, N_CHANNELS + c, np.int32)
    loads = dict(gains=dict(zone=every, chan=full(0), factor=rng.uniform(0.5, 1.5, Z)),
                 flows=dict(zone=every, volume_chan=full(1), temp_chan=full(2), volume_gain=rng.uniform(0.5, 1.5, Z)),
                 thermostats=dict(sensor_zone=every, target_zone=every, heat_chan=full(3), cool_chan=np.full(Z, -1, np.int32),
                                  heat_power=rng.uniform(200.0, 2000.0, Z), cool_power=np.zeros(Z), band=np.full(Z, 0.5)))
    # the rows leg C carries: the gains and flows by the rule of include/heat_amd.h, computed before the clock starts
    tk = channel[:, N_CHANNELS + 2:N_CHANNELS + 3] + 273.15
    mcp = (101325. * 28.97 / (8314.46261815324 * tk) * (loads["flows"]["volume_gain"] * channel[:, N_CHANNELS + 1:N_CHANNELS + 2])) * (
        1002.7370 + 1.2324e-2 * tk)
    rows_a0 = loads["gains"]["factor"] * channel[:, N_CHANNELS:N_CHANNELS + 1] + mcp * channel[:, N_CHANNELS + 2:N_CHANNELS + 3]
    rows_b0 = mcp
if IDEAL:
    # one more channel, the cooling setpoint (C); every zone held between the heating setpoint of leg D's thermostats and it
    channel = np.concatenate([channel, rng.uniform(24.0, 26.0, (STEPS, 1))], axis=1)
    ideal = dict(zone=every, heat_chan=full(3), cool_chan=full(4))

    def leg_i(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads, ideal=ideal, **drives)
        dt = time.perf_counter() - t0
        assert out["failed_step"] == -1 and np.all(np.isfinite(out["ideal_q"])) and np.all(np.isfinite(out["trace"]))
        return dt * 1e3 / steps
if SKY or SHADES:
    FRONT = ("solar_front", "ir_front")
    azimuth = rng.uniform(0.0, 2.0 * np.pi, S)
    sun = skym.sun_direction(172, 24.0 * np.arange(STEPS) / STEPS, np.radians(48.0))
    up = np.maximum(sun[:, 2], 0.0)
    beam, diffuse = np.where(sun[:, 2] > 0.0, 800.0, 0.0), 60.0 + 140.0 * up
    record = np.stack([sun[:, 0], sun[:, 1], sun[:, 2], beam, diffuse, 0.2 * (beam * up + diffuse), np.full(STEPS, 350.0),
                       np.full(STEPS, 420.0)], axis=1)[:, None, :]
    sky_args = dict(mode=np.full(S, 1 | 4, np.uint8), normals=(np.cos(azimuth), np.sin(azimuth), np.zeros(S)))
    not_driven = np.full(S, -1, np.int32)

    def leg_cp(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                       **{k: drives[k] for k in FRONT})
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace))
        return dt * 1e3 / steps

    def leg_k(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                       sky=dict(sky_args, record=record[:steps]), **{k: (not_driven, drives[k][1]) for k in FRONT})
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace))
        return dt * 1e3 / steps
if SHADES:
    # one shade per wall, in the wall's plane: a window of 1.2 m x 1.5 m under an overhang, between two fins, behind a horizon
    wall_normal = sky_args["normals"]
    wall_right, wall_up = shm.frame_of(wall_normal)
    shade_args = dict(surface=np.arange(S), normal=wall_normal, right=wall_right, up=wall_up, width=rng.uniform(0.8, 2.4, S),
                      height=rng.uniform(1.0, 2.0, S), overhang_depth=rng.uniform(0.3, 0.9, S), overhang_gap=rng.uniform(0.0, 0.3, S),
                      fin_pos_depth=rng.uniform(0.1, 0.5, S), fin_pos_gap=rng.uniform(0.0, 0.2, S), fin_neg_depth=rng.uniform(0.1, 0.5, S),
                      fin_neg_gap=rng.uniform(0.0, 0.2, S), diffuse_factor=rng.uniform(0.6, 0.9, S), ground_factor=rng.uniform(0.8, 1.0, S),
                      horizon=np.zeros(S, np.int32), horizon_tan2=shm.horizon_tan2(rng.uniform(0.0, 12.0, (1, 16))),
                      front_shade=np.arange(S, dtype=np.int32))
    SHADE_BYTES = dict(k_series_shading_per_shade=19 * 8 + 2 * 4, gathered_in_k_series_sky_per_shaded_side=4 + 3 * 8)  # 160 + 28

    def leg_s(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, lit = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                            sky=dict(sky_args, record=record[:steps]), shades=shade_args, sunlit=False,
                                                            **{k: (not_driven, drives[k][1]) for k in FRONT})
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace))
        return dt * 1e3 / steps
if BLINDS:
    # three more channels (a position schedule, an enable schedule, a cooling setpoint C) and a blind on every shade, of four
    # kinds in turn: scheduled; controlled by the irradiance; gated by the wall's zone; gated and with an enable schedule
    c_bl = channel.shape[1]
    channel = np.concatenate([channel, rng.uniform(-0.2, 1.2, (STEPS, 1)), np.where(np.arange(STEPS) % 8 < 6, 1.0, 0.0)[:, None],
                              rng.uniform(19.5, 20.5, (STEPS, 1))], axis=1)
    kind = np.arange(S) % 4
    wall_zone = np.where(md["back_kind"] == mdl.SPACE, md["back_zone"], md["front_zone"]).astype(np.int32)
    blind_args = dict(shade=np.arange(S, dtype=np.int32), beam_closed=rng.uniform(0.05, 0.3, S), diffuse_closed=rng.uniform(0.1, 0.4, S),
                      ground_closed=rng.uniform(0.1, 0.4, S), pos_chan=np.where(kind == 0, c_bl, -1).astype(np.int32),
                      irr_close=rng.uniform(150.0, 400.0, S), irr_open=rng.uniform(50.0, 150.0, S),
                      zone=np.where(kind >= 2, np.clip(wall_zone, 0, Z - 1), -1).astype(np.int32),
                      set_chan=np.where(kind >= 2, c_bl + 2, -1).astype(np.int32), band=np.full(S, 0.5),
                      enable_chan=np.where(kind == 3, c_bl + 1, -1).astype(np.int32))
    # per shade: blind_of_shade, site, f, five table rows, three effective factors; per blind: four integers, six reals, the
    # state byte, three accumulators read and written; the record, the channels and the zone temperature are shared
    BLIND_BYTES = dict(k_series_blinds_per_shade=4 + 4 + 8 + 5 * 8 + 3 * 8, k_series_blinds_per_blind=4 * 4 + 6 * 8 + 1 + 3 * 16)

    def leg_bl(b, w, n_sub, steps, aniso=None):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, lit, bl = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                                sky=dict(sky_args, record=record[:steps]), shades=shade_args, sunlit=False,
                                                                blinds=blind_args, position=False, blind_incident=False,
                                                                aniso=None if aniso is None else dict(aniso, coef=aniso["coef"][:steps]),
                                                                **{k: (not_driven, drives[k][1]) for k in FRONT})
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace)) and bl["steps_closed"].any()
        # (a whole day: the sun comes and goes, controlled blinds switch; a short series may lie in the night)
        assert steps < STEPS or bl["switches"].any()
        return dt * 1e3 / steps
if ANISO:
    # Reindl's coefficients of the day's records and Reindl's band of every wall and shade (vertical planes); per consumer lane one
    # 16-byte pair beside the record and one band
    circ, horiz = skym.reindl(record[:, 0, :], 172)
    wall_band = skym.band_reindl(sky_args["normals"])
    aniso_args = dict(coef=np.stack([circ, horiz], axis=1)[:, None, :], front_band=wall_band, shade_band=wall_band)
    ANISO_BYTES = dict(per_sky_driven_side=8, per_shade_with_a_blind=8, per_site_and_step=16)

    def leg_an(b, w, n_sub, steps):
        return leg_bl(b, w, n_sub, steps, aniso_args)
if COMFORT:
    # three more channels (occupancy: nine steps in twenty-four; an adaptive band that drifts with the steps) and one sensor per
    # zone over the sides that face it, area-weighted, every one the control temperature of its zone: the thermostats sense it
    c_cf = channel.shape[1]
    drift = 0.5 * np.sin(2.0 * np.pi * np.arange(STEPS) / 24.0)
    channel = np.concatenate([channel, np.where(np.arange(STEPS) % 24 < 9, 1.0, 0.0)[:, None], (20.0 + drift)[:, None], (24.0 + drift)[:, None]], axis=1)
    comfort_args = dict(cfm.by_area(md, air_weight=0.5, control=True), occ_chan=np.full(Z, c_cf, np.int32), lo_chan=np.full(Z, c_cf + 1, np.int32),
                        hi_chan=np.full(Z, c_cf + 2, np.int32))
    # per entry: face index, weight and the gathered node; per sensor: two offsets, four integers, the air weight, the zone
    # temperature, `top`, twelve accumulators read and written; per zone: the control sensor, a gather and a store
    COMFORT_BYTES = dict(k_series_comfort_per_entry=4 + 8 + 8, k_series_comfort_per_sensor=8 + 4 * 4 + 8 + 8 + 8 + 12 * 16, k_series_control_T_per_zone=4 + 8 + 8)

    def leg_cf(b, w, n_sub, steps, comfort="given"):
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads, aniso={},
                             comfort=comfort_args if comfort == "given" else comfort, operative=False, mrt=False, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0]))
        assert comfort is None or (out[4]["n_occupied"] > 0).all()
        return dt * 1e3 / steps
if HANDLERS:
    # five more channels (outdoor air, the bypass setpoint of the extract air, the minimum and the maximum supply temperature,
    # the volume flow of a branch) and one unit for every five zones: five balanced branches, a bypass and both coils
    c_ah = channel.shape[1]
    channel = np.concatenate([channel, rng.uniform(-5.0, 30.0, (STEPS, 1)), rng.uniform(21.0, 25.0, (STEPS, 1)), rng.uniform(16.0, 18.0, (STEPS, 1)),
                              rng.uniform(22.0, 26.0, (STEPS, 1)), rng.uniform(0.01, 0.05, (STEPS, 1))], axis=1)
    NU = max(1, Z // 5)
    handler_args = ahm.concat(*[ahm.balanced(np.arange(5 * u, min(5 * u + 5, Z)), c_ah + 4, c_ah, eff_gain=0.8, bypass_chan=c_ah + 1, bypass_band=0.5,
                                             bypass_min_delta=0.5, heat_chan=c_ah + 2, cool_chan=c_ah + 3, heat_cap=2000.0, cool_cap=1500.0)
                                for u in range(NU)])

    def leg_ah(b, w, n_sub, steps, handlers="given"):
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                             handlers=handler_args if handlers == "given" else handlers, supply_t=False, recovered=False, coil_q=False,
                             branch_q=False, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0]))
        assert handlers is None or np.all(np.isfinite(out[4]["sum_branch_q"]))
        return dt * 1e3 / steps
if SPECIES:
    # four more channels (the outdoor levels of the two species, a source strength, a limit) and per zone one demand vent on
    # the first species — outdoor air at the handlers' outdoor temperature — and one source of each species
    c_sp = channel.shape[1]
    channel = np.concatenate([channel, rng.uniform(400.0, 450.0, (STEPS, 1)), rng.uniform(4.0, 9.0, (STEPS, 1)), rng.uniform(0.0, 1.0, (STEPS, 1)),
                              rng.uniform(900.0, 1100.0, (STEPS, 1))], axis=1)
    species_args = dict(outdoor_chan=aspm.per_zone([c_sp, c_sp + 1], Z), conc=np.stack([rng.uniform(400.0, 1500.0, Z), rng.uniform(4.0, 12.0, Z)]),
                        src_zone=np.tile(every, 2), src_species=np.repeat([0, 1], Z), src_chan=np.full(2 * Z, c_sp + 2, np.int32),
                        src_factor=np.concatenate([rng.uniform(0.5, 3.0, Z), rng.uniform(0.005, 0.03, Z)]), vent_zone=every,
                        vent_species=np.zeros(Z, np.int32), vent_temp_chan=np.full(Z, c_ah, np.int32), vent_v_min=np.zeros(Z),
                        vent_v_max=rng.uniform(0.02, 0.1, Z), vent_c_lo=rng.uniform(500.0, 700.0, Z), vent_c_hi=rng.uniform(900.0, 1200.0, Z),
                        limit_chan=np.array([c_sp + 3, -1], np.int32))

    def leg_sp(b, w, n_sub, steps, species="given"):
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads, handlers=handler_args, supply_t=False,
                             recovered=False, coil_q=False, branch_q=False, species=species_args if species == "given" else species,
                             conc_rows=False, vent_v=False, vent_q=False, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0]))
        assert species == {} or (np.all(np.isfinite(out[5]["conc"])) and out[5]["sum_volume"].any())
        return dt * 1e3 / steps
if OPENINGS:
    # three more channels (the wind speed at the openings, an open fraction that leaves [0, 1] at times, the windows' setpoint)
    # and the derived columns: per zone one opening to outside air at the handlers' outdoor temperature (wind and stack, or
    # single-sided, in turn) feeding a controlled supply path of that zone, per pair of zones (2j, 2j + 1) one doorway
    c_op = channel.shape[1]
    n_door = Z // 2
    NO = Z + n_door
    channel = np.concatenate([channel, rng.uniform(0.2, 6.0, (STEPS, 1)), rng.uniform(-0.2, 1.3, (STEPS, 1)), rng.uniform(18.0, 24.0, (STEPS, 1)),
                              np.full((STEPS, NO), np.nan)], axis=1)
    c_der = c_op + 3
    area = rng.uniform(0.02, 0.08, Z)
    ws, ss = opm.wind_and_stack(area, 0.6, rng.uniform(0.25, 0.6, Z), rng.uniform(0.3, 1.2, Z)), opm.single_sided(area, rng.uniform(0.8, 1.6, Z))
    single = np.arange(Z) % 2 == 1
    dw = opm.doorway(rng.uniform(0.7, 1.0, n_door), rng.uniform(1.9, 2.2, n_door), 0.6)
    opening_args = opm.concat(
        dict(zone_a=every, zone_b=np.full(Z, -1), temp_chan=np.full(Z, c_ah), wind_chan=np.full(Z, c_op), frac_chan=np.full(Z, c_op + 1),
             area=np.where(single, ss["area"], ws["area"]), cw=np.where(single, ss["cw"], ws["cw"]), cs=np.where(single, 0.0, ws["cs"]),
             ca=np.where(single, ss["ca"], 0.0), c0=np.where(single, ss["c0"], 0.0)),
        dict(zone_a=2 * np.arange(n_door), zone_b=2 * np.arange(n_door) + 1, area=0.1 * dw["area"], cs=dw["cs"], c0=np.full(n_door, 0.01)))
    opening_args["out_chan"] = (c_der + np.arange(NO)).astype(np.int32)
    air_args = apm.concat(dict(target=every, source=np.full(Z, -1), temp_chan=np.full(Z, c_ah), volume_chan=c_der + np.arange(Z),
                               open_chan=np.full(Z, c_op + 2), sense=np.ones(Z, np.int8), band=np.full(Z, 0.5), min_delta=np.full(Z, 0.5)),
                          apm.doorway(2 * np.arange(n_door), 2 * np.arange(n_door) + 1, c_der + Z + np.arange(n_door)))
    # per opening: six integers, five reals, two gathered temperatures, up to three values of the row, V into the row, and the three
    # accumulators read and written
    OPENING_BYTES = dict(k_series_openings_per_opening=6 * 4 + 5 * 8 + 2 * 8 + 3 * 8 + 8 + 3 * 16)

    def leg_op(b, w, n_sub, steps, openings="given", table=None, rows=False):
        table = channel if table is None else table
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=table[:steps], probes=probes, loads=loads, air=air_args, path_q=False, handlers=handler_args,
                             supply_t=False, recovered=False, coil_q=False, branch_q=False, species=species_args, conc_rows=False, vent_v=False,
                             vent_q=False, openings=opening_args if openings == "given" else openings, opening_v=rows, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[6]["conc"]))
        assert openings is None or (np.all(np.isfinite(out[7]["sum_v"])) and out[7]["sum_v"].any())
        return (dt * 1e3 / steps, out) if rows else dt * 1e3 / steps
if CONTROLLERS:
    # two more channels (a heating and a cooling setpoint) and the derived columns: per zone one proportional valve on the zone's
    # air feeding one more gain of the zone loads, per opening one PI loop on the air of its zone_a, cooling action, feeding the
    # opening's open fraction (the openings then read a controller's column: the controllers are the first kernel of the step)
    c_ct = channel.shape[1]
    NCT = Z + NO
    channel = np.concatenate([channel, rng.uniform(19.0, 23.0, (STEPS, 1)), rng.uniform(20.0, 24.0, (STEPS, 1)), np.full((STEPS, NCT), np.nan)], axis=1)
    controller_args = ctm.concat(
        dict(sense_index=every, set_chan=np.full(Z, c_ct), out_hi=rng.uniform(200.0, 1500.0, Z), **ctm.proportional(rng.uniform(1.0, 4.0, Z))),
        dict(sense_index=opening_args["zone_a"], set_chan=np.full(NO, c_ct + 1), action=np.full(NO, -1), out_hi=np.ones(NO),
             **ctm.pi(rng.uniform(2.0, 6.0, NO), 8.0)))
    controller_args["out_chan"] = (c_ct + 2 + np.arange(NCT)).astype(np.int32)
    loads_ct = dict(loads, gains=dict(zone=np.concatenate([every, every]), chan=np.concatenate([loads["gains"]["chan"], controller_args["out_chan"][:Z]]),
                                      factor=np.concatenate([loads["gains"]["factor"], np.ones(Z)])))
    opening_ct = dict(opening_args, frac_chan=controller_args["out_chan"][Z:])
    # per controller: eight integers, seven reals, the sensed temperature, the setpoint, the state read and written, out into the
    # row, and the two sums and two of the counts read and written
    CONTROLLER_BYTES = dict(k_series_controllers_per_controller=8 * 4 + 7 * 8 + 2 * 8 + (8 + 1) * 2 + 8 + 4 * 16)

    def leg_ct(b, w, n_sub, steps, controllers="given", table=None, rows=False):
        table = channel if table is None else table
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=table[:steps], probes=probes, loads=loads_ct, air=air_args, path_q=False, handlers=handler_args,
                             supply_t=False, recovered=False, coil_q=False, branch_q=False, species=species_args, conc_rows=False, vent_v=False,
                             vent_q=False, openings=opening_ct, opening_v=False, controllers=controller_args if controllers == "given" else controllers,
                             control_u=False, control_out=rows, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[6]["conc"])) and np.all(np.isfinite(out[7]["sum_v"]))
        assert controllers is None or (np.all(np.isfinite(out[8]["sum_u"])) and out[8]["sum_u"].any())
        return (dt * 1e3 / steps, out) if rows else dt * 1e3 / steps
if NETWORKS:
    # two more channels (the wind pressures of two facades) and the derived columns: per building of ten zones one network — a chain of
    # doorways, every other one a tall opening of two links, one link to outside per zone at its storey's height; the first of a
    # building never closes, the others follow the openings' open-fraction schedule — and the air paths that read every column
    c_nw = channel.shape[1]
    PER = 10
    NB = Z // PER
    zi = np.arange(NB * PER)
    local = zi % PER
    door = zi[local > 0]
    tall = (local[local > 0] % 2 == 1)
    t = anm.tall_opening(rng.uniform(0.7, 1.0, len(door)), rng.uniform(1.9, 2.2, len(door)), 0.6, sill=3.0 * (local[local > 0] // 5))
    d_a = np.concatenate([door, door[tall]])
    d_b = np.concatenate([door - 1, door[tall] - 1])
    d_c = np.concatenate([np.where(tall, t["c"][0], anm.orifice(rng.uniform(0.005, 0.03, len(door)), 0.6)), t["c"][1][tall]])
    d_gh = np.concatenate([t["gh"][0], t["gh"][1][tall]])
    n_in, n_out = len(d_a), len(zi)
    network_args = dict(net_offset=(PER * np.arange(NB + 1)).astype(np.int32), tol=np.full(NB, 1e-7), max_iter=np.full(NB, 24, np.int32),
                        g_min=np.full(NB, 1e-9), node_zone=zi.astype(np.int32), zone_a=np.concatenate([d_a, zi]).astype(np.int32),
                        zone_b=np.concatenate([d_b, np.full(n_out, -1)]).astype(np.int32),
                        temp_chan=np.concatenate([np.full(n_in, -1), np.full(n_out, c_ah)]).astype(np.int32),
                        wp_chan=np.concatenate([np.full(n_in, -1), c_nw + zi % 2]).astype(np.int32),
                        frac_chan=np.concatenate([np.full(n_in, -1), np.where(local == 0, -1, c_op + 1)]).astype(np.int32),
                        c=np.concatenate([d_c, anm.orifice(rng.uniform(0.004, 0.04, n_out), 0.6)]),
                        gh=np.concatenate([d_gh, anm.G * (3.0 * (local // 5) + rng.uniform(0.3, 2.6, n_out))]), p_lin=np.full(n_in + n_out, 0.05))
    NL = n_in + n_out
    network_args["out_ab"] = np.concatenate([c_nw + 2 + np.arange(n_in), np.full(n_out, -1)]).astype(np.int32)
    network_args["out_ba"] = (c_nw + 2 + n_in + np.arange(NL)).astype(np.int32)
    channel = np.concatenate([channel, rng.uniform(-6.0, 6.0, (STEPS, 2)), np.full((STEPS, n_in + NL), np.nan)], axis=1)
    network_paths = anm.paths(network_args)
    air_nw = apm.concat(air_args, {k: v for k, v in network_paths.items() if k != "link"})

    def leg_nw(b, w, n_sub, steps, networks="given", table=None, rows=False):
        table = channel if table is None else table
        b.synchronize()
        t0 = time.perf_counter()
        out = b.march_series(w[:steps], n_sub, channel=table[:steps], probes=probes, loads=loads_ct, air=air_nw, path_q=False, handlers=handler_args,
                             supply_t=False, recovered=False, coil_q=False, branch_q=False, species=species_args, conc_rows=False, vent_v=False,
                             vent_q=False, openings=opening_ct, opening_v=False, controllers=controller_args, control_u=False, control_out=False,
                             networks=network_args if networks == "given" else networks, link_q=rows, node_p=False, net_iters=rows, **drives)
        dt = time.perf_counter() - t0
        assert out[1] == -1 and np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[6]["conc"])) and np.all(np.isfinite(out[7]["sum_v"]))
        assert networks is None or (np.all(np.isfinite(out[9]["sum_ba"])) and out[9]["sum_ba"].any() and not out[9]["unconverged"].any())
        return (dt * 1e3 / steps, out) if rows else dt * 1e3 / steps
if RADIATION:
    # every back a receiver of the backs of its room, area-weighted; its long-wave channel goes (an input has one source)
    exchange = rrm.exchange_by_area(md)
    assert np.all(exchange["rc_side"] == 1) and len(exchange["rc_surface"]) == S
    not_driven = np.full(S, -1, np.int32)
    RADIATION_BYTES = dict(k_series_emission_per_emitter=4 + 8 + 8, k_series_room_radiation_per_entry=4 + 8 + 8,
                           k_series_room_radiation_per_receiver=4 + 4 + 8 + 8)   # face + T + E; src + factor + E; rec + off + gain + rad_t

    def leg_r(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, irr, total = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                                   radiation=exchange, irradiance=False,
                                                                   **dict(drives, ir_back=(not_driven, drives["ir_back"][1])))
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(total)) and np.all(total > 0)
        return dt * 1e3 / steps
if AMBIENT:
    # four more channels (ground, two neighbours, outdoor air; C); half of the sides mixed with the next zone's temperature
    c_amb = channel.shape[1]
    channel = np.concatenate([channel, rng.uniform(8.0, 14.0, (STEPS, 1)), rng.uniform(16.0, 24.0, (STEPS, 2)), rng.uniform(-5.0, 30.0, (STEPS, 1))], axis=1)
    NB = len(ambient_walls)
    mixes = np.arange(NB) % 2 == 1
    ambient_args = dict(surface=ambient_walls, side=np.ones(NB, np.uint8), chan=(c_amb + np.where(mixes, 3, np.arange(NB) % 3)).astype(np.int32),
                        gain=rng.uniform(0.9, 1.1, NB), offset=rng.uniform(-1.0, 1.0, NB),
                        mix_zone=np.where(mixes, (md["back_zone"][ambient_walls] + 1) % Z, -1).astype(np.int32),
                        mix=np.where(mixes, ambm.b_factor(0.5), 0.0))
    AMBIENT_BYTES = dict(per_side=4 + 4 + 4 + 8 + 8 + 4 + 8 + 8 + 8, per_mixing_side_more=8)   # rec, peer, chan, gain, offset, mix zone, mix, sum (read + write: 16), the record's field; the zone

    def leg_m(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, amb_t, total = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                                     ambient=ambient_args, ambient_t=False, **drives)
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(total))
        return dt * 1e3 / steps
if GAINS:
    assert np.all(np.diff(md["back_zone"]) >= 0) and np.all(md["back_kind"] == mdl.SPACE)
    sun = skym.sun_direction(172, 24.0 * np.arange(STEPS) / STEPS, np.radians(48.0))
    up = np.maximum(sun[:, 2], 0.0)
    beam, diffuse = np.where(sun[:, 2] > 0.0, 800.0, 0.0), 60.0 + 140.0 * up
    record = np.stack([sun[:, 0], sun[:, 1], sun[:, 2], beam, diffuse, 0.2 * (beam * up + diffuse), np.full(STEPS, 350.0),
                       np.full(STEPS, 420.0)], axis=1)[:, None, :]
    first_of = np.searchsorted(md["back_zone"], np.arange(Z + 1))
    rank_in_zone = np.arange(S) - first_of[md["back_zone"]]
    is_ap = rank_in_zone % 10 == 0
    windows, receivers = np.flatnonzero(is_ap), np.flatnonzero(~is_ap)
    NA, NR = len(windows), len(receivers)
    ap_of_zone = [np.flatnonzero(is_ap[first_of[z]:first_of[z + 1]]) + first_of[z] for z in range(Z)]
    ap_index = np.cumsum(is_ap) - 1                                        # wall -> its aperture number
    per_zone = np.array([len(a) for a in ap_of_zone])
    R_MAX = int(per_zone.max())
    # rank j of every receiver: the j-th aperture of its zone (-1: the zone has fewer)
    ap_rank = np.full((R_MAX, NR), -1, np.int64)
    for j in range(R_MAX):
        has = per_zone[md["back_zone"][receivers]] > j
        zr = md["back_zone"][receivers][has]
        ap_rank[j, has] = ap_index[np.array([a[j] if len(a) > j else -1 for a in ap_of_zone])[zr]]
    zone_area = np.bincount(md["back_zone"], weights=md["area"], minlength=Z)
    share_b = rng.uniform(0.5, 1.5, (R_MAX, NR)) / zone_area[md["back_zone"][receivers]]
    share_d = rng.uniform(0.5, 1.5, (R_MAX, NR)) / zone_area[md["back_zone"][receivers]]
    on = ap_rank >= 0
    # the caller's list, aperture-major (as distribute_by_area gives it): the library sorts it by receiver
    order = np.argsort(ap_rank[on], kind="stable")
    gains_args = dict(ap_surface=windows, ap_normal=(md["normal_x"][windows], md["normal_y"][windows], md["cos_tilt"][windows]),
                      ap_tau_coef=np.concatenate([rng.uniform(0.3, 0.8, (NA, 1)), rng.uniform(-0.05, 0.05, (NA, 5))], axis=1),
                      ap_tau_diffuse=rng.uniform(0.3, 0.7, NA), ap_scale=md["area"][windows],
                      en_surface=np.broadcast_to(receivers, ap_rank.shape)[on][order], en_side=np.ones(int(on.sum()), np.uint8),
                      en_aperture=ap_rank[on][order].astype(np.int32), en_beam=share_b[on][order], en_diffuse=share_d[on][order])
    NE = int(on.sum())
    back_chan_j = drives["solar_back"][0].copy()
    back_chan_j[receivers] = -1
    back_chan_h = drives["solar_back"][0].copy()
    back_chan_h[receivers] = channel.shape[1] + np.arange(NR)
    # the bytes a step of k_series_solar_gains moves: per table element the aperture number, the share pair and the gathered
    # (Pb, Pd); per receiver its record number, gain, absorptance factor, slot number, the mirror and the SideDyn field
    rows = np.zeros((NR + 63) // 64 * 64, np.int64)
    rows[:NR] = on.sum(axis=0)[np.argsort(receivers, kind="stable")]
    padded = int(rows.reshape(-1, 64).max(axis=1).sum() * 64)
    gains_bytes = dict(entries=NE, table_elements_with_padding=padded, per_element=4 + 16 + 16, receivers=NR, per_receiver=4 + 8 + 8 + 8 + 8 + 8,
                       total=int(padded * 36 + NR * 44))
    # the bytes a step of k_series_inputs moves in leg J: 160 per wall with all four inputs driven (16 of channel
    # numbers, 72 per side), 40 less for a receiver, whose back solar input it leaves alone (gain, absorptance factor, slot
    # number read; the mirror and the SideDyn field written)
    inputs_bytes = dict(per_wall_all_four_driven=160, per_receiver=120, total=int(160 * NA + 120 * NR))

    def host_columns(steps):
        """What the host of leg H computes per series: the rule of solar_gains.transmitted / received over the prepared ranks."""
        pb, pd = sgm.transmitted(record[:steps, 0][:, None, :], gains_args["ap_normal"], gains_args["ap_tau_coef"],
                                 gains_args["ap_tau_diffuse"], gains_args["ap_scale"])
        cols = np.zeros((steps, NR))
        for k in range(steps):
            v = np.zeros(NR)
            for j in range(R_MAX):
                a = ap_rank[j]
                v = v + np.where(a >= 0, share_b[j] * pb[k, a], 0.0)
                v = v + np.where(a >= 0, share_d[j] * pd[k, a], 0.0)
            cols[k] = v
        return cols

    def leg_h(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        wide = np.concatenate([channel[:steps], host_columns(steps)], axis=1)
        t1 = time.perf_counter()
        trace, failed, applied, modes = b.march_series(w[:steps], n_sub, channel=wide, probes=probes, loads=loads,
                                                       **dict(drives, solar_back=(back_chan_h, drives["solar_back"][1])))
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace))
        return dt * 1e3 / steps, (t1 - t0) * 1e3 / steps

    def leg_j(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, transmitted, ap_sum = b.march_series(
            w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads, sky=dict(record=record[:steps]), gains=gains_args,
            **dict(drives, solar_back=(back_chan_j, drives["solar_back"][1])))
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(transmitted))
        return dt * 1e3 / steps
if AIR:
    # three more channels: the volume through a doorway, through a vent (m3/s), the vents' cooling setpoint (C); the supply
    # air of a vent is leg D's outdoor temperature channel
    c_air = channel.shape[1]
    channel = np.concatenate([channel, rng.uniform(0.02, 0.10, (STEPS, 1)), rng.uniform(0.0, 0.05, (STEPS, 1)),
                              rng.uniform(19.0, 23.0, (STEPS, 1))], axis=1)
    left = np.flatnonzero((np.arange(Z) % 10 != 9) & (np.arange(Z) + 1 < Z)).astype(np.int32)
    doors = apm.doorway(left, left + 1, c_air, rng.uniform(0.5, 1.5, len(left)))
    vents = dict(target=np.arange(Z, dtype=np.int32), source=np.full(Z, -1, np.int32), temp_chan=np.full(Z, N_CHANNELS + 2, np.int32),
                 volume_chan=np.full(Z, c_air + 1, np.int32), volume_gain=rng.uniform(0.5, 1.5, Z), open_chan=np.full(Z, c_air + 2, np.int32),
                 sense=np.ones(Z, np.int8), band=np.full(Z, 0.5), min_delta=np.full(Z, 1.0))
    air_args = apm.concat(doors, vents)
    NP = len(air_args["target"])

    def leg_air(b, w, n_sub, steps):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, air = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads,
                                                            air=air_args, **drives)
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(air["path_q"]))
        return dt * 1e3 / steps, air
if REPORT:
    # the envelope of zone z: both faces of the walls whose back faces it (uniform_massive: all of a zone's walls, contiguous)
    assert np.all(np.diff(md["back_zone"]) >= 0) and np.all(md["back_kind"] == mdl.SPACE)
    walls_of = np.searchsorted(md["back_zone"], np.arange(Z + 1))
    env_slots = np.concatenate([np.concatenate([md["flow_front_slot"][a:e], md["flow_back_slot"][a:e]]) for a, e in zip(walls_of[:-1], walls_of[1:])])
    env_weights = np.concatenate([np.tile(md["area"][a:e], 2) for a, e in zip(walls_of[:-1], walls_of[1:])])
    env_off = 2 * walls_of.astype(np.int64)
    inside_nodes = md["first_node_slot"] + np.diff(md["node_offset"]) - 1
    HOT = 26.0
    TH = ("steps_heating", "steps_cooling", "switches", "sum_heating", "sum_cooling")
    zone_groups = dict(offset=env_off, slot=env_slots, weight=env_weights)
    one_group = dict(offset=np.array([0, len(env_slots)]), slot=env_slots, weight=env_weights)

    def report_of(n_probes, groups, stats):
        Q = n_probes + len(groups["offset"]) - 1
        hi = np.full(Q, np.nan)
        hi[:Z] = HOT
        return dict(groups=groups, stats=stats, limits=dict(hi=hi) if "n_above" in stats else None, thermostat_stats=TH)

    def leg_e(b, w, n_sub, steps):
        """Trace everything, reduce on the host."""
        b.synchronize()
        t0 = time.perf_counter()
        pr = np.concatenate([probes, env_slots])
        trace, failed, applied, modes = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=pr, loads=loads, **drives)
        t1 = time.perf_counter()
        zt = trace[:, :Z]
        out = dict(q_min=zt.min(axis=0), q_max=zt.max(axis=0), q_sum=np.add.accumulate(zt, axis=0)[-1], q_n_above=(zt > HOT).sum(axis=0),
                   envelope=np.add.reduceat(trace[:, Z:] * env_weights, env_off[:-1], axis=1))
        mode = np.where(applied > 0, 1, np.where(applied < 0, 2, 0))
        before = np.concatenate([np.zeros((1, Z), mode.dtype), mode[:-1]])
        out.update(th_steps_heating=(mode == 1).sum(axis=0), th_steps_cooling=(mode == 2).sum(axis=0), th_switches=(mode != before).sum(axis=0),
                   th_sum_heating=np.add.accumulate(np.where(applied > 0, applied, 0.0), axis=0)[-1],
                   th_sum_cooling=np.add.accumulate(np.where(applied < 0, applied, 0.0), axis=0)[-1])
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(out["envelope"]))
        return dt * 1e3 / steps, (t1 - t0) * 1e3 / steps, out

    def leg_f(b, w, n_sub, steps, pr=probes, groups=zone_groups, stats=("min", "max", "sum", "n_above")):
        b.synchronize()
        t0 = time.perf_counter()
        trace, failed, applied, modes, out = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=pr, loads=loads,
                                                            report=report_of(len(pr), groups, stats), trace=False, applied=False, **drives)
        dt = time.perf_counter() - t0
        assert failed == -1 and np.all(np.isfinite(out["q_min"]))
        return dt * 1e3 / steps, out

    def leg_g(b, w, n_sub, steps, stats=("min",)):
        return leg_f(b, w, n_sub, steps, pr=np.concatenate([probes, inside_nodes]), stats=stats)


def leg_a(b, state, w, n_sub, steps):
    """(ms per step in the calls alone, ms per step with numpy's writes)"""
    in_calls, t_all = 0.0, time.perf_counter()
    for k in range(steps):
        for key in KEYS:
            chan, gain = drives[key]
            state[md[key + "_slot"]] = gain * channel[k, chan]
        t0 = time.perf_counter()
        b.march(state, w[k], outputs=b.OUT_SCALARS | b.OUT_ZONES)
        in_calls += time.perf_counter() - t0
    return in_calls * 1e3 / steps, (time.perf_counter() - t_all) * 1e3 / steps


def leg_b(b, w, steps):
    b.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        b.march_resident(w[k])
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def leg_c(b, w, n_sub, steps):
    b.synchronize()
    t0 = time.perf_counter()
    trace, failed = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, **drives)
    dt = time.perf_counter() - t0
    assert failed == -1 and np.all(np.isfinite(trace))
    return dt * 1e3 / steps


def leg_rows(b, w, n_sub, steps):
    b.synchronize()
    t0 = time.perf_counter()
    trace, failed = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, zone_a0=rows_a0[:steps],
                                   zone_b0=rows_b0[:steps], **drives)
    dt = time.perf_counter() - t0
    assert failed == -1 and np.all(np.isfinite(trace))
    return dt * 1e3 / steps


def leg_d(b, w, n_sub, steps):
    b.synchronize()
    t0 = time.perf_counter()
    trace, failed, applied, modes = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, loads=loads, **drives)
    dt = time.perf_counter() - t0
    assert failed == -1 and np.all(np.isfinite(trace))
    return dt * 1e3 / steps


result = dict(model="uniform_massive(%d, 32, Z=%d)" % (S, md["n_zones"]), channels=int(channel.shape[1]), steps=STEPS, rounds=ROUNDS,
              probes=int(len(probes)), legs={})
with HeatBatch(md) as b:
    state = st0.copy()
    b.upload_state(state)
    if IDEAL:
        bs = HeatBatch(md, no_fusion=True)
        bs.upload_state(state)
    for n_sub in ((2,) if ONE else (2, 20)):
        w = mdl.weather_series(STEPS * n_sub, 45.0).reshape(STEPS, n_sub, 3)
        if COMFORT:
            leg_cf(b, w, n_sub, min(STEPS, 10), None)  # warm-up
            leg_cf(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with comfort: C %.3f ms per step" % leg_cf(b, w, n_sub, STEPS))
                continue
            nn, cc, nn1, cc1 = [], [], [], []
            for r in range(ROUNDS):
                nn.append(leg_cf(b, w, n_sub, STEPS, None))
                cc.append(leg_cf(b, w, n_sub, STEPS))
                nn1.append(leg_cf(b, w, n_sub, 1, None))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                cc1.append(leg_cf(b, w, n_sub, 1))
            N_, C_, N1, C1 = (float(np.median(v)) for v in (nn, cc, nn1, cc1))
            Ns, Cs = (N_ * STEPS - N1) / (STEPS - 1), (C_ * STEPS - C1) / (STEPS - 1)  # per step once the call is set up
            NE = len(comfort_args["en_sensor"])
            nbytes = COMFORT_BYTES["k_series_comfort_per_entry"] * NE + COMFORT_BYTES["k_series_comfort_per_sensor"] * Z + COMFORT_BYTES["k_series_control_T_per_zone"] * Z
            result["legs"]["n_sub=%d" % n_sub] = dict(
                N_comfort_null_ms=N_, C_comfort_ms=C_, C_minus_N_ms=C_ - N_, C_over_N=C_ / N_, N_series_of_one_step_ms=N1,
                C_series_of_one_step_ms=C1, C_minus_N_series_of_one_step_ms=C1 - N1, N_without_setup_ms=Ns, C_without_setup_ms=Cs,
                C_minus_N_without_setup_ms=Cs - Ns, sensors=int(Z), entries=int(NE), bytes=COMFORT_BYTES,
                bytes_per_step_of_the_two_kernels=int(nbytes), all_rounds=dict(N=nn, C=cc, N_one_step=nn1, C_one_step=cc1))
            print("n_sub %2d: N comfort NULL %.3f ms/step, C comfort %.3f -> C - N = %+.3f ms, C / N = %.4f; a series of one step: "
                  "N %.2f ms, C %.2f ms -> per step without the set-up N %.3f, C %.3f, C - N = %+.3f (%d sensors, %d entries, %d steps, "
                  "median of %d rounds)" % (n_sub, N_, C_, C_ - N_, C_ / N_, N1, C1, Ns, Cs, Cs - Ns, Z, NE, STEPS, ROUNDS), flush=True)
            continue
        if NETWORKS:
            # the flows of one W series into ordinary channels: leg F's table (the state is uploaded anew before every series of this
            # mode, so that F and W march the same steps from the same start)
            def fresh(leg, *a, **kw):
                b.upload_state(state)
                return leg(b, w, n_sub, *a, **kw)
            _, first = fresh(leg_nw, STEPS, rows=True)  # (warm-up as well)
            q = first[9]["link_q"]
            fed = channel.copy()
            ab, ba = network_args["out_ab"], network_args["out_ba"]
            fed[:, ab[ab >= 0]] = np.where(q > 0, q, 0.0)[:, ab >= 0]
            fed[:, ba[ba >= 0]] = np.where(q < 0, -q, 0.0)[:, ba >= 0]
            _, same = fresh(leg_nw, STEPS, None, fed, rows=True)
            assert np.array_equal(first[0], same[0]), "the series with the flows fed back marches other bits"
            if ONE:
                print("one series with networks: W %.3f ms per step" % fresh(leg_nw, STEPS))
                continue
            ff, ww, ff1, ww1 = [], [], [], []
            for r in range(ROUNDS):
                ff.append(fresh(leg_nw, STEPS, None, fed))
                ww.append(fresh(leg_nw, STEPS))
                ff1.append(fresh(leg_nw, 1, None, fed))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                ww1.append(fresh(leg_nw, 1))
            F_, W_, F1, W1 = (float(np.mean(v)) for v in (ff, ww, ff1, ww1))
            Fs, Ws = (F_ * STEPS - F1) / (STEPS - 1), (W_ * STEPS - W1) / (STEPS - 1)  # per step once the call is set up
            its = first[9]["net_iters"]
            result["legs"]["n_sub=%d" % n_sub] = dict(
                F_flows_fed_back_ms=F_, W_networks_ms=W_, W_minus_F_ms=W_ - F_, W_over_F=W_ / F_, F_spread_ms=[min(ff), max(ff)],
                W_spread_ms=[min(ww), max(ww)], F_series_of_one_step_ms=F1, W_series_of_one_step_ms=W1, W_minus_F_series_of_one_step_ms=W1 - F1,
                F_without_setup_ms=Fs, W_without_setup_ms=Ws, W_minus_F_without_setup_ms=Ws - Fs, networks=int(NB), nodes=int(NB * PER),
                links=int(NL), nodes_per_network=PER, lanes_per_network=next(w for w in (8, 16, 32, 64) if PER <= w), channels=int(channel.shape[1]), iterations_mean=float(its.mean()),
                iterations_max=int(its.max()), traces_equal=True, all_rounds=dict(F=ff, W=ww, F_one_step=ff1, W_one_step=ww1))
            print("n_sub %2d: F flows fed back %.3f ms/step (%.3f-%.3f), W networks %.3f (%.3f-%.3f) -> W - F = %+.3f ms, W / F = %.4f; a series of "
                  "one step: F %.2f ms, W %.2f ms -> per step without the set-up F %.3f, W %.3f, W - F = %+.3f (%d networks, %d nodes, %d links, "
                  "%.1f iterations a solve, at most %d; %d steps, mean of %d rounds)" % (
                      n_sub, F_, min(ff), max(ff), W_, min(ww), max(ww), W_ - F_, W_ / F_, F1, W1, Fs, Ws, Ws - Fs, NB, NB * PER, NL, its.mean(),
                      its.max(), STEPS, ROUNDS), flush=True)
            continue
        if CONTROLLERS:
            # the outputs of one K series into ordinary channels: leg P's table (the state is uploaded anew before every series of
            # this mode, so that P and K march the same steps from the same start)
            def fresh(leg, *a, **kw):
                b.upload_state(state)
                return leg(b, w, n_sub, *a, **kw)
            _, first = fresh(leg_ct, STEPS, rows=True)  # (warm-up as well)
            precomputed = channel.copy()
            precomputed[:, controller_args["out_chan"]] = first[8]["control_out"]
            _, same = fresh(leg_ct, STEPS, None, precomputed, rows=True)
            assert np.array_equal(first[0], same[0]), "the series with the outputs precomputed marches other bits"
            if ONE:
                print("one series with controllers: K %.3f ms per step" % fresh(leg_ct, STEPS))
                continue
            pp, kk, pp1, kk1 = [], [], [], []
            for r in range(ROUNDS):
                pp.append(fresh(leg_ct, STEPS, None, precomputed))
                kk.append(fresh(leg_ct, STEPS))
                pp1.append(fresh(leg_ct, 1, None, precomputed))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                kk1.append(fresh(leg_ct, 1))
            P_, K_, P1, K1 = (float(np.median(v)) for v in (pp, kk, pp1, kk1))
            Ps, Ks = (P_ * STEPS - P1) / (STEPS - 1), (K_ * STEPS - K1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                P_outputs_precomputed_ms=P_, K_controllers_ms=K_, K_minus_P_ms=K_ - P_, K_over_P=K_ / P_, P_series_of_one_step_ms=P1,
                K_series_of_one_step_ms=K1, K_minus_P_series_of_one_step_ms=K1 - P1, P_without_setup_ms=Ps, K_without_setup_ms=Ks,
                K_minus_P_without_setup_ms=Ks - Ps, controllers=int(NCT), openings=int(NO), channels=int(channel.shape[1]),
                bytes=CONTROLLER_BYTES, bytes_per_step_of_k_series_controllers=int(CONTROLLER_BYTES["k_series_controllers_per_controller"] * NCT),
                traces_equal=True, all_rounds=dict(P=pp, K=kk, P_one_step=pp1, K_one_step=kk1))
            print("n_sub %2d: P outputs precomputed %.3f ms/step, K controllers %.3f -> K - P = %+.3f ms, K / P = %.4f; a series of one step: "
                  "P %.2f ms, K %.2f ms -> per step without the set-up P %.3f, K %.3f, K - P = %+.3f (%d controllers, %d openings, %d steps, "
                  "median of %d rounds)" % (n_sub, P_, K_, K_ - P_, K_ / P_, P1, K1, Ps, Ks, Ks - Ps, NCT, NO, STEPS, ROUNDS), flush=True)
            continue
        if OPENINGS:
            # the flows of one O series into ordinary channels: leg C's table (the state is uploaded anew before every series
            # of this mode, so that C and O march the same steps from the same start)
            def fresh(leg, *a, **kw):
                b.upload_state(state)
                return leg(b, w, n_sub, *a, **kw)
            _, first = fresh(leg_op, STEPS, rows=True)  # (warm-up as well)
            precomputed = channel.copy()
            precomputed[:, opening_args["out_chan"]] = first[7]["opening_v"]
            _, same = fresh(leg_op, STEPS, None, precomputed, rows=True)
            assert np.array_equal(first[0], same[0]), "the series with the flows precomputed marches other bits"
            if ONE:
                print("one series with openings: O %.3f ms per step" % fresh(leg_op, STEPS))
                continue
            cc, oo, cc1, oo1 = [], [], [], []
            for r in range(ROUNDS):
                cc.append(fresh(leg_op, STEPS, None, precomputed))
                oo.append(fresh(leg_op, STEPS))
                cc1.append(fresh(leg_op, 1, None, precomputed))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                oo1.append(fresh(leg_op, 1))
            C_, O_, C1, O1 = (float(np.median(v)) for v in (cc, oo, cc1, oo1))
            Cs, Os = (C_ * STEPS - C1) / (STEPS - 1), (O_ * STEPS - O1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                C_flows_precomputed_ms=C_, O_openings_ms=O_, O_minus_C_ms=O_ - C_, O_over_C=O_ / C_, C_series_of_one_step_ms=C1,
                O_series_of_one_step_ms=O1, O_minus_C_series_of_one_step_ms=O1 - C1, C_without_setup_ms=Cs, O_without_setup_ms=Os,
                O_minus_C_without_setup_ms=Os - Cs, openings=int(NO), paths=int(Z + 2 * n_door), channels=int(channel.shape[1]),
                bytes=OPENING_BYTES, bytes_per_step_of_k_series_openings=int(OPENING_BYTES["k_series_openings_per_opening"] * NO),
                traces_equal=True, all_rounds=dict(C=cc, O=oo, C_one_step=cc1, O_one_step=oo1))
            print("n_sub %2d: C flows precomputed %.3f ms/step, O openings %.3f -> O - C = %+.3f ms, O / C = %.4f; a series of one step: "
                  "C %.2f ms, O %.2f ms -> per step without the set-up C %.3f, O %.3f, O - C = %+.3f (%d openings, %d paths, %d steps, "
                  "median of %d rounds)" % (n_sub, C_, O_, O_ - C_, O_ / C_, C1, O1, Cs, Os, Os - Cs, NO, Z + 2 * n_door, STEPS, ROUNDS), flush=True)
            continue
        if SPECIES:
            leg_sp(b, w, n_sub, min(STEPS, 10), {})  # warm-up
            leg_sp(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with air species: P %.3f ms per step" % leg_sp(b, w, n_sub, STEPS))
                continue
            nn, pp, nn1, pp1 = [], [], [], []
            for r in range(ROUNDS):
                nn.append(leg_sp(b, w, n_sub, STEPS, {}))
                pp.append(leg_sp(b, w, n_sub, STEPS))
                nn1.append(leg_sp(b, w, n_sub, 1, {}))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                pp1.append(leg_sp(b, w, n_sub, 1))
            N_, P_, N1, P1 = (float(np.median(v)) for v in (nn, pp, nn1, pp1))
            Ns, Ps = (N_ * STEPS - N1) / (STEPS - 1), (P_ * STEPS - P1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                N_species_null_ms=N_, P_species_ms=P_, P_minus_N_ms=P_ - N_, P_over_N=P_ / N_, N_series_of_one_step_ms=N1,
                P_series_of_one_step_ms=P1, P_minus_N_series_of_one_step_ms=P1 - N1, N_without_setup_ms=Ns, P_without_setup_ms=Ps,
                P_minus_N_without_setup_ms=Ps - Ns, species=2, lanes=int(2 * Z), vents=int(Z), sources=int(2 * Z),
                all_rounds=dict(N=nn, P=pp, N_one_step=nn1, P_one_step=pp1))
            print("n_sub %2d: N species NULL %.3f ms/step, P species %.3f -> P - N = %+.3f ms, P / N = %.4f; a series of one step: "
                  "N %.2f ms, P %.2f ms -> per step without the set-up N %.3f, P %.3f, P - N = %+.3f (%d lanes, %d vents, %d steps, "
                  "median of %d rounds)" % (n_sub, N_, P_, P_ - N_, P_ / N_, N1, P1, Ns, Ps, Ps - Ns, 2 * Z, Z, STEPS, ROUNDS), flush=True)
            continue
        if HANDLERS:
            leg_ah(b, w, n_sub, min(STEPS, 10), {})  # warm-up
            leg_ah(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with air handlers: H %.3f ms per step" % leg_ah(b, w, n_sub, STEPS))
                continue
            nn, hh, nn1, hh1 = [], [], [], []
            for r in range(ROUNDS):
                nn.append(leg_ah(b, w, n_sub, STEPS, {}))
                hh.append(leg_ah(b, w, n_sub, STEPS))
                nn1.append(leg_ah(b, w, n_sub, 1, {}))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                hh1.append(leg_ah(b, w, n_sub, 1))
            N_, H_, N1, H1 = (float(np.median(v)) for v in (nn, hh, nn1, hh1))
            Ns, Hs = (N_ * STEPS - N1) / (STEPS - 1), (H_ * STEPS - H1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                N_handlers_null_ms=N_, H_handlers_ms=H_, H_minus_N_ms=H_ - N_, H_over_N=H_ / N_, N_series_of_one_step_ms=N1,
                H_series_of_one_step_ms=H1, H_minus_N_series_of_one_step_ms=H1 - N1, N_without_setup_ms=Ns, H_without_setup_ms=Hs,
                H_minus_N_without_setup_ms=Hs - Ns, units=int(NU), branches=int(len(handler_args["br_unit"])),
                all_rounds=dict(N=nn, H=hh, N_one_step=nn1, H_one_step=hh1))
            print("n_sub %2d: N handlers NULL %.3f ms/step, H handlers %.3f -> H - N = %+.3f ms, H / N = %.4f; a series of one step: "
                  "N %.2f ms, H %.2f ms -> per step without the set-up N %.3f, H %.3f, H - N = %+.3f (%d units, %d branches, %d steps, "
                  "median of %d rounds)" % (n_sub, N_, H_, H_ - N_, H_ / N_, N1, H1, Ns, Hs, Hs - Ns, NU, len(handler_args["br_unit"]), STEPS, ROUNDS),
                  flush=True)
            continue
        if IDEAL:
            leg_i(bs, w, n_sub, min(STEPS, 10))  # warm-up
            if ONE:
                print("one series with ideal loads: %.3f ms per step" % leg_i(bs, w, n_sub, STEPS))
                continue
            leg_d(bs, w, n_sub, min(STEPS, 10))
            leg_d(b, w, n_sub, min(STEPS, 10))

            def leg_r(steps):
                b.set_ideal_resident(True)
                assert b.ideal_resident == 1, "the batch of leg D is not eligible for resident ideal loads"
                launches = b.n_fused_launches
                ms = leg_i(b, w, n_sub, steps)
                assert b.n_fused_launches > launches, "leg R was streamed"
                b.set_ideal_resident(False)
                return ms
            leg_r(min(STEPS, 10))
            ss, ii, rr, dd = [], [], [], []
            for r in range(ROUNDS):
                ss.append(leg_d(bs, w, n_sub, STEPS))
                ii.append(leg_i(bs, w, n_sub, STEPS))
                rr.append(leg_r(STEPS))
                dd.append(leg_d(b, w, n_sub, STEPS))
            Sm, Im, Rm, Dm = float(np.median(ss)), float(np.median(ii)), float(np.median(rr)), float(np.median(dd))
            result["legs"]["n_sub=%d" % n_sub] = dict(
                S_streamed_series_with_loads_ms=Sm, I_ideal_series_ms=Im, R_resident_ideal_series_ms=Rm, D_series_with_loads_ms=Dm,
                I_minus_S_ms=Im - Sm, I_minus_S_per_sub_timestep_us=(Im - Sm) * 1e3 / n_sub, I_over_S=Im / Sm, I_over_D=Im / Dm,
                R_minus_D_ms=Rm - Dm, R_minus_D_per_sub_timestep_us=(Rm - Dm) * 1e3 / n_sub, R_over_D=Rm / Dm, R_over_I=Rm / Im,
                ideal_loads=int(Z), all_rounds=dict(S=ss, I=ii, R=rr, D=dd))
            print("n_sub %2d: S streamed series with loads %.3f ms/step, I with ideal loads %.3f, R the same resident %.3f, D fused %.3f -> "
                  "I - S = %.3f ms (%.1f us per sub-timestep), I / S = %.3f, I / D = %.3f, R / D = %.3f, R / I = %.3f (%d steps, median of "
                  "%d rounds)" % (n_sub, Sm, Im, Rm, Dm, Im - Sm, (Im - Sm) * 1e3 / n_sub, Im / Sm, Im / Dm, Rm / Dm, Rm / Im, STEPS, ROUNDS),
                  flush=True)
            continue
        if RADIATION:
            leg_d(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_r(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with room radiation: R %.3f ms per step" % leg_r(b, w, n_sub, STEPS))
                continue
            d, rr, d1, rr1 = [], [], [], []
            for r in range(ROUNDS):
                d.append(leg_d(b, w, n_sub, STEPS))
                rr.append(leg_r(b, w, n_sub, STEPS))
                d1.append(leg_d(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                rr1.append(leg_r(b, w, n_sub, 1))
            D, R, D1, R1 = (float(np.median(v)) for v in (d, rr, d1, rr1))
            Ds, Rs = (D * STEPS - D1) / (STEPS - 1), (R * STEPS - R1) / (STEPS - 1)  # per step once the call is set up
            NE, NM = len(exchange["en_receiver"]), S
            nbytes = (RADIATION_BYTES["k_series_emission_per_emitter"] * NM + RADIATION_BYTES["k_series_room_radiation_per_entry"] * NE +
                      RADIATION_BYTES["k_series_room_radiation_per_receiver"] * S)
            result["legs"]["n_sub=%d" % n_sub] = dict(
                D_channel_driven_ms=D, R_room_radiation_ms=R, R_minus_D_ms=R - D, R_over_D=R / D, D_series_of_one_step_ms=D1,
                R_series_of_one_step_ms=R1, R_minus_D_series_of_one_step_ms=R1 - D1, D_without_setup_ms=Ds, R_without_setup_ms=Rs,
                R_minus_D_without_setup_ms=Rs - Ds, receivers=int(S), emitters=int(NM), entries=int(NE), bytes=RADIATION_BYTES,
                bytes_per_step_of_the_two_kernels=int(nbytes), all_rounds=dict(D=d, R=rr, D_one_step=d1, R_one_step=rr1))
            print("n_sub %2d: D channel-driven %.3f ms/step, R room radiation %.3f -> R - D = %+.3f ms, R / D = %.4f; a series of one "
                  "step: D %.2f ms, R %.2f ms -> per step without the set-up D %.3f, R %.3f, R - D = %+.3f (%d entries, %d steps, median "
                  "of %d rounds)" % (n_sub, D, R, R - D, R / D, D1, R1, Ds, Rs, Rs - Ds, NE, STEPS, ROUNDS), flush=True)
            continue
        if AMBIENT:
            leg_d(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_m(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with an ambient drive: M %.3f ms per step" % leg_m(b, w, n_sub, STEPS))
                continue
            n, m, n1, m1 = [], [], [], []
            for r in range(ROUNDS):
                n.append(leg_d(b, w, n_sub, STEPS))
                m.append(leg_m(b, w, n_sub, STEPS))
                n1.append(leg_d(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                m1.append(leg_m(b, w, n_sub, 1))
            N_, M_, N1, M1 = (float(np.median(v)) for v in (n, m, n1, m1))
            Ns, Ms = (N_ * STEPS - N1) / (STEPS - 1), (M_ * STEPS - M1) / (STEPS - 1)  # per step once the call is set up
            nbytes = AMBIENT_BYTES["per_side"] * NB + AMBIENT_BYTES["per_mixing_side_more"] * int(mixes.sum())
            result["legs"]["n_sub=%d" % n_sub] = dict(
                N_drive_null_ms=N_, M_ambient_drive_ms=M_, M_minus_N_ms=M_ - N_, M_over_N=M_ / N_, N_series_of_one_step_ms=N1,
                M_series_of_one_step_ms=M1, N_without_setup_ms=Ns, M_without_setup_ms=Ms, M_minus_N_without_setup_ms=Ms - Ns,
                driven_sides=int(NB), mixing_sides=int(mixes.sum()), bytes=AMBIENT_BYTES, bytes_per_step_of_k_series_ambient=int(nbytes),
                all_rounds=dict(N=n, M=m, N_one_step=n1, M_one_step=m1))
            print("n_sub %2d: N drive NULL %.3f ms/step, M ambient drive %.3f -> M - N = %+.3f ms, M / N = %.4f; a series of one step: "
                  "N %.2f ms, M %.2f ms -> per step without the set-up N %.3f, M %.3f, M - N = %+.3f (%d driven sides, %d steps, median of "
                  "%d rounds)" % (n_sub, N_, M_, M_ - N_, M_ / N_, N1, M1, Ns, Ms, Ms - Ns, NB, STEPS, ROUNDS), flush=True)
            continue
        if ANISO:
            leg_bl(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_an(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with blinds under an anisotropic sky: A %.3f ms per step" % leg_an(b, w, n_sub, STEPS))
                continue
            bl, an, bl1, an1 = [], [], [], []
            for r in range(ROUNDS):
                bl.append(leg_bl(b, w, n_sub, STEPS))
                an.append(leg_an(b, w, n_sub, STEPS))
                bl1.append(leg_bl(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                an1.append(leg_an(b, w, n_sub, 1))
            B, A, B1, A1 = (float(np.median(v)) for v in (bl, an, bl1, an1))
            Bs, As = (B * STEPS - B1) / (STEPS - 1), (A * STEPS - A1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                B_aniso_null_ms=B, A_aniso_ms=A, A_minus_B_ms=A - B, A_over_B=A / B, B_series_of_one_step_ms=B1,
                A_series_of_one_step_ms=A1, A_minus_B_series_of_one_step_ms=A1 - B1, B_without_setup_ms=Bs, A_without_setup_ms=As,
                A_minus_B_without_setup_ms=As - Bs, sky_driven_sides=int(S), shades=int(S), blinds=int(S), bytes=ANISO_BYTES,
                all_rounds=dict(B=bl, A=an, B_one_step=bl1, A_one_step=an1))
            print("n_sub %2d: B aniso NULL %.3f ms/step, A aniso %.3f -> A - B = %+.3f ms, A / B = %.4f; a series of one step: "
                  "B %.2f ms, A %.2f ms -> per step without the set-up B %.3f, A %.3f, A - B = %+.3f (%d sides and blinds, %d steps, "
                  "median of %d rounds)" % (n_sub, B, A, A - B, A / B, B1, A1, Bs, As, As - Bs, S, STEPS, ROUNDS), flush=True)
            continue
        if BLINDS:
            leg_s(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_bl(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with blinds: B %.3f ms per step" % leg_bl(b, w, n_sub, STEPS))
                continue
            sh, bl, sh1, bl1 = [], [], [], []
            for r in range(ROUNDS):
                sh.append(leg_s(b, w, n_sub, STEPS))
                bl.append(leg_bl(b, w, n_sub, STEPS))
                sh1.append(leg_s(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                bl1.append(leg_bl(b, w, n_sub, 1))
            Sh, B, Sh1, B1 = (float(np.median(v)) for v in (sh, bl, sh1, bl1))
            Ss, Bs = (Sh * STEPS - Sh1) / (STEPS - 1), (B * STEPS - B1) / (STEPS - 1)  # per step once the call is set up
            nbytes = (BLIND_BYTES["k_series_blinds_per_shade"] + BLIND_BYTES["k_series_blinds_per_blind"]) * S
            result["legs"]["n_sub=%d" % n_sub] = dict(
                S_blinds_null_ms=Sh, B_blinds_ms=B, B_minus_S_ms=B - Sh, B_over_S=B / Sh, S_series_of_one_step_ms=Sh1,
                B_series_of_one_step_ms=B1, S_without_setup_ms=Ss, B_without_setup_ms=Bs, B_minus_S_without_setup_ms=Bs - Ss,
                shades=int(S), blinds=int(S), bytes=BLIND_BYTES, bytes_per_step_of_k_series_blinds=int(nbytes),
                all_rounds=dict(S=sh, B=bl, S_one_step=sh1, B_one_step=bl1))
            print("n_sub %2d: S blinds NULL %.3f ms/step, B blinds %.3f -> B - S = %+.3f ms, B / S = %.4f; a series of one step: "
                  "S %.2f ms, B %.2f ms -> per step without the set-up S %.3f, B %.3f, B - S = %+.3f (%d blinds, %d steps, median of "
                  "%d rounds)" % (n_sub, Sh, B, B - Sh, B / Sh, Sh1, B1, Ss, Bs, Bs - Ss, S, STEPS, ROUNDS), flush=True)
            continue
        if SHADES:
            leg_k(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_s(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with shades: S %.3f ms per step" % leg_s(b, w, n_sub, STEPS))
                continue
            k, sh, k1, sh1 = [], [], [], []
            for r in range(ROUNDS):
                k.append(leg_k(b, w, n_sub, STEPS))
                sh.append(leg_s(b, w, n_sub, STEPS))
                k1.append(leg_k(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                sh1.append(leg_s(b, w, n_sub, 1))
            K, Sh, K1, Sh1 = (float(np.median(v)) for v in (k, sh, k1, sh1))
            Ks, Ss = (K * STEPS - K1) / (STEPS - 1), (Sh * STEPS - Sh1) / (STEPS - 1)  # per step once the call is set up
            per_shade = SHADE_BYTES["k_series_shading_per_shade"] + SHADE_BYTES["gathered_in_k_series_sky_per_shaded_side"]
            bound_ms = 1.5 * per_shade * S / 2.0e12 * 1e3
            result["legs"]["n_sub=%d" % n_sub] = dict(
                K_sky_ms=K, S_shaded_ms=Sh, S_minus_K_ms=Sh - K, S_over_K=Sh / K, K_series_of_one_step_ms=K1, S_series_of_one_step_ms=Sh1,
                S_minus_K_series_of_one_step_ms=Sh1 - K1, K_without_setup_ms=Ks, S_without_setup_ms=Ss, S_minus_K_without_setup_ms=Ss - Ks,
                expectation_bound_ms=bound_ms, expectation_S_minus_K_within_the_bound=bool(Sh - K <= bound_ms),
                expectation_S_minus_K_without_setup_within_the_bound=bool(Ss - Ks <= bound_ms), shades=int(S), bytes=SHADE_BYTES,
                all_rounds=dict(K=k, S=sh, K_one_step=k1, S_one_step=sh1))
            print("n_sub %2d: K sky %.3f ms/step, S shaded %.3f -> S - K = %+.3f ms (bound %.3f), S / K = %.4f; a series of one step: "
                  "K %.2f ms, S %.2f ms -> per step without the set-up K %.3f, S %.3f, S - K = %+.3f (%d steps, median of %d rounds)" % (
                      n_sub, K, Sh, Sh - K, bound_ms, Sh / K, K1, Sh1, Ks, Ss, Ss - Ks, STEPS, ROUNDS), flush=True)
            continue
        if SKY:
            leg_cp(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_k(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series of each: C' channels %.3f ms per step, K sky %.3f" % (leg_cp(b, w, n_sub, STEPS), leg_k(b, w, n_sub, STEPS)))
                continue
            c, k, c1, k1 = [], [], [], []
            for r in range(ROUNDS):
                c.append(leg_cp(b, w, n_sub, STEPS))
                k.append(leg_k(b, w, n_sub, STEPS))
                c1.append(leg_cp(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                k1.append(leg_k(b, w, n_sub, 1))
            Cc, K, C1, K1 = float(np.median(c)), float(np.median(k)), float(np.median(c1)), float(np.median(k1))
            Cs, Ks = (Cc * STEPS - C1) / (STEPS - 1), (K * STEPS - K1) / (STEPS - 1)  # per step once the call is set up
            result["legs"]["n_sub=%d" % n_sub] = dict(
                C_prime_channels_ms=Cc, K_sky_ms=K, K_over_C_prime=K / Cc, K_minus_C_prime_ms=K - Cc,
                expectation_K_within_5_percent_of_C_prime=bool(K <= 1.05 * Cc),
                C_prime_series_of_one_step_ms=C1, K_series_of_one_step_ms=K1, C_prime_without_setup_ms=Cs, K_without_setup_ms=Ks,
                K_over_C_prime_without_setup=Ks / Cs,
                table_bytes_per_step=dict(C_prime_as_measured=int(8 * channel.shape[1]), C_prime_with_a_column_per_wall_input=int(8 * 2 * S),
                                          K_records=64),
                all_rounds=dict(C_prime=c, K=k, C_prime_one_step=c1, K_one_step=k1))
            print("n_sub %2d: C' channels %.3f ms/step, K sky %.3f -> K / C' = %.4f, K - C' = %+.3f ms; a series of one step: C' %.2f ms, "
                  "K %.2f ms -> per step without the set-up C' %.3f, K %.3f, K / C' = %.4f (%d steps, median of %d rounds)" % (
                      n_sub, Cc, K, K / Cc, K - Cc, C1, K1, Cs, Ks, Ks / Cs, STEPS, ROUNDS), flush=True)
            continue
        if GAINS:
            leg_j(b, w, n_sub, min(STEPS, 10))  # warm-up
            if ONE:
                print("one series with gains: J %.3f ms per step" % leg_j(b, w, n_sub, STEPS))
                continue
            leg_h(b, w, n_sub, min(STEPS, 10))
            leg_d(b, w, n_sub, min(STEPS, 10))
            h, hh, j, d, h1, j1, d1 = [], [], [], [], [], [], []
            for r in range(ROUNDS):
                x, y = leg_h(b, w, n_sub, STEPS)
                h.append(x), hh.append(y)
                j.append(leg_j(b, w, n_sub, STEPS))
                d.append(leg_d(b, w, n_sub, STEPS))  # the same series without the receivers: their input from the 64 shared channels
                h1.append(leg_h(b, w, n_sub, 1)[0])  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                j1.append(leg_j(b, w, n_sub, 1))
                d1.append(leg_d(b, w, n_sub, 1))
            H, HH, J, D, H1, J1, D1 = (float(np.median(v)) for v in (h, hh, j, d, h1, j1, d1))
            # per step once the call is set up. A series of one step carries the WHOLE set-up of J and D (tables that do not
            # grow with the steps) but only one 7.2 MB row of H's [steps] x 7.2 MB table: H_without_setup still holds H's
            # upload, so J is set against D here, not against H
            Hs, Js, Ds = ((x * STEPS - x1) / (STEPS - 1) for x, x1 in ((H, H1), (J, J1), (D, D1)))
            result["legs"]["n_sub=%d" % n_sub] = dict(
                H_channel_columns_ms=H, H_host_columns_alone_ms=HH, J_gains_ms=J, D_no_receivers_ms=D, J_over_H=J / H,
                J_over_H_without_the_hosts_columns=J / (H - HH),
                expectation_J_at_most_1_05_H=bool(J <= 1.05 * H), H_series_of_one_step_ms=H1, J_series_of_one_step_ms=J1,
                D_series_of_one_step_ms=D1, H_without_its_first_row_ms=Hs, J_without_setup_ms=Js, D_without_setup_ms=Ds,
                J_minus_D_without_setup_ms=Js - Ds, expectation_J_within_5_percent_of_D_plus_230_us=bool(Js <= 1.05 * (Ds + 0.230)),
                table_bytes_per_step=dict(H_channel_row=int(8 * (channel.shape[1] + NR)), J_records=64),
                apertures=NA, receivers=NR, k_series_solar_gains_bytes_per_step=gains_bytes, k_series_inputs_bytes_per_step_in_J=inputs_bytes,
                all_rounds=dict(H=h, H_host_columns=hh, J=j, D=d, H_one_step=h1, J_one_step=j1, D_one_step=d1))
            print("n_sub %2d: H channel columns %.3f ms/step (%.3f of it the host's columns), J gains %.3f, D without the receivers %.3f "
                  "-> J / H = %.4f (%.4f of H without the host's columns); a series of one step: H %.2f ms, J %.2f ms, D %.2f ms -> per step "
                  "without the set-up J %.3f, D %.3f, J - D = %+.3f (H without its first row %.3f) (%d steps, median of %d rounds)" % (
                      n_sub, H, HH, J, D, J / H, J / (H - HH), H1, J1, D1, Js, Ds, Js - Ds, Hs, STEPS, ROUNDS), flush=True)
            continue
        if AIR:
            leg_air(b, w, n_sub, min(STEPS, 10))  # warm-up
            if ONE:
                print("one series with air paths: A %.3f ms per step" % leg_air(b, w, n_sub, STEPS)[0])
                continue
            leg_d(b, w, n_sub, min(STEPS, 10))
            d, a, d1, a1 = [], [], [], []
            for r in range(ROUNDS):
                d.append(leg_d(b, w, n_sub, STEPS))
                x, air = leg_air(b, w, n_sub, STEPS)
                a.append(x)
                d1.append(leg_d(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (checks, tables, uploads) + a step
                a1.append(leg_air(b, w, n_sub, 1)[0])
            D, A, D1, A1 = (float(np.median(v)) for v in (d, a, d1, a1))
            Ds, As = (D * STEPS - D1) / (STEPS - 1), (A * STEPS - A1) / (STEPS - 1)  # per step once the call is set up
            vent = air_args["open_chan"] >= 0
            result["legs"]["n_sub=%d" % n_sub] = dict(
                D_series_with_loads_ms=D, A_series_with_air_paths_ms=A, A_minus_D_ms=A - D, A_over_D=A / D,
                D_series_of_one_step_ms=D1, A_series_of_one_step_ms=A1, A_minus_D_series_of_one_step_ms=A1 - D1,
                D_without_setup_ms=Ds, A_without_setup_ms=As, A_minus_D_without_setup_ms=As - Ds,
                paths=NP, paths_per_zone=NP / Z, controlled=int(vent.sum()),
                last_series=dict(vent_steps_open_share=float(air["steps_open"][vent].mean() / STEPS),
                                 vents_that_switched=int((air["switches"][vent] > 0).sum())),
                all_rounds=dict(D=d, A=a, D_one_step=d1, A_one_step=a1))
            print("n_sub %2d: D loads %.3f ms/step, A with %d air paths %.3f -> A - D = %+.3f ms, A / D = %.4f; a series of one step: "
                  "D %.2f ms, A %.2f ms -> per step without the set-up D %.3f, A %.3f, A - D = %+.3f; vents open in %.0f %% of their "
                  "steps, %d of %d switched (%d steps, median of %d rounds)" % (
                      n_sub, D, NP, A, A - D, A / D, D1, A1, Ds, As, As - Ds, 100 * air["steps_open"][vent].mean() / STEPS,
                      int((air["switches"][vent] > 0).sum()), int(vent.sum()), STEPS, ROUNDS), flush=True)
            continue
        if REPORT:
            if ONE:
                leg = dict(zones=leg_f, nodes=leg_g)
                run = (lambda n: leg_f(b, w, n_sub, n, groups=one_group)[0]) if REPORT == "one-group" else (lambda n: leg[REPORT](b, w, n_sub, n)[0])
                run(min(STEPS, 10))  # warm-up
                print("one series with a report (%s): %.3f ms per step" % (REPORT, run(STEPS)))
                continue
            leg_d(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_f(b, w, n_sub, min(STEPS, 10))
            leg_e(b, w, n_sub, min(STEPS, 10))
            d, e, e_dev, f, g, g4, f1, d1 = [], [], [], [], [], [], [], []
            for r in range(ROUNDS):
                d.append(leg_d(b, w, n_sub, STEPS))
                x, y, host = leg_e(b, w, n_sub, STEPS)
                e.append(x), e_dev.append(y)
                x, dev = leg_f(b, w, n_sub, STEPS)
                f.append(x)
                g.append(leg_g(b, w, n_sub, STEPS)[0])
                g4.append(leg_g(b, w, n_sub, STEPS, stats=("min", "max", "sum", "n_above"))[0])
                f1.append(leg_f(b, w, n_sub, 1)[0])
                d1.append(leg_d(b, w, n_sub, 1))
            # (the legs march on from one another's state, so host and device numbers are of different steps: not compared here;
            # tests/test_series_report_gpu.py compares them)
            med = lambda v: float(np.median(v))
            result["legs"]["n_sub=%d" % n_sub] = dict(
                D_series_with_loads_ms=med(d), E_trace_and_numpy_ms=med(e), E_march_and_trace_alone_ms=med(e_dev), F_report_ms=med(f),
                G_report_and_node_min_ms=med(g), G4_report_and_four_node_statistics_ms=med(g4), F_series_of_one_step_ms=med(f1),
                F_without_setup_ms=(med(f) * STEPS - med(f1)) / (STEPS - 1), D_series_of_one_step_ms=med(d1),
                D_without_setup_ms=(med(d) * STEPS - med(d1)) / (STEPS - 1),
                F_over_D=med(f) / med(d), E_over_F=med(e) / med(f), G_minus_F_ms=med(g) - med(f), G4_minus_F_ms=med(g4) - med(f),
                quantities=dict(F=int(2 * Z), G=int(2 * Z + S)), group_entries=int(len(env_slots)),
                all_rounds=dict(D=d, E=e, E_march_and_trace=e_dev, F=f, G=g, G4=g4, F_one_step=f1, D_one_step=d1))
            print("n_sub %2d: D loads %.3f ms/step, E trace + numpy %.3f (%.3f before numpy), F report %.3f -> F / D = %.3f, E / F = %.1f; "
                  "G %.3f, G4 %.3f; a series of one step: F %.2f ms, D %.2f ms -> per step without the set-up F %.3f, D %.3f "
                  "(%d steps, median of %d rounds)" % (
                      n_sub, med(d), med(e), med(e_dev), med(f), med(f) / med(d), med(e) / med(f), med(g), med(g4), med(f1), med(d1),
                      (med(f) * STEPS - med(f1)) / (STEPS - 1), (med(d) * STEPS - med(d1)) / (STEPS - 1), STEPS, ROUNDS),
                  flush=True)
            continue
        if LOADS:
            leg_rows(b, w, n_sub, min(STEPS, 10))  # warm-up
            leg_d(b, w, n_sub, min(STEPS, 10))
            if ONE:
                print("one series with loads: %.3f ms per step" % leg_d(b, w, n_sub, STEPS))
                continue
            c, d, c1, d1 = [], [], [], []
            for r in range(ROUNDS):
                c.append(leg_rows(b, w, n_sub, STEPS))
                d.append(leg_d(b, w, n_sub, STEPS))
                c1.append(leg_rows(b, w, n_sub, 1))
                d1.append(leg_d(b, w, n_sub, 1))
            Cc, D, C1, D1 = float(np.median(c)), float(np.median(d)), float(np.median(c1)), float(np.median(d1))
            result["legs"]["n_sub=%d" % n_sub] = dict(
                C_series_with_rows_ms=Cc, D_series_with_loads_ms=D, D_over_C=D / Cc, C_series_of_one_step_ms=C1,
                D_series_of_one_step_ms=D1, all_rounds=dict(C=c, D=d, C_one_step=c1, D_one_step=d1))
            print("n_sub %2d: C series with rows %.3f ms/step, D series with loads %.3f -> D / C = %.3f; a series of one step: "
                  "C %.2f ms, D %.2f ms (%d steps, median of %d rounds)" % (n_sub, Cc, D, D / Cc, C1, D1, STEPS, ROUNDS), flush=True)
            continue
        leg_c(b, w, n_sub, min(STEPS, 10))  # warm-up
        if ONE:
            print("one series: %.3f ms per step" % leg_c(b, w, n_sub, STEPS))
            continue
        leg_b(b, w, 5)
        leg_a(b, state, w, n_sub, 3)
        a, a_np, bb, c, c1 = [], [], [], [], []
        for r in range(ROUNDS):
            x, y = leg_a(b, state, w, n_sub, min(STEPS, 50))
            a.append(x), a_np.append(y)
            bb.append(leg_b(b, w, STEPS))
            c.append(leg_c(b, w, n_sub, STEPS))
            c1.append(leg_c(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (tables built and uploaded) + a step
        A, A_np, B, Cc, C1 = float(np.median(a)), float(np.median(a_np)), float(np.median(bb)), float(np.median(c)), float(np.median(c1))
        steady = (Cc * STEPS - C1) / (STEPS - 1) - B  # what a step costs over the floor once the call is set up
        result["legs"]["n_sub=%d" % n_sub] = dict(
            A_per_call_ms=A, A_with_numpy_writes_ms=A_np, B_resident_ms=B, C_series_ms=Cc, C_over_A=Cc / A, C_minus_B_ms=Cc - B,
            C_series_of_one_step_ms=C1, C_minus_B_without_setup_ms=steady, all_rounds=dict(A=a, A_with_numpy=a_np, B=bb, C=c, C_one_step=c1))
        print("n_sub %2d: A per-call %.3f ms/step (%.3f with numpy's writes), B resident %.3f, C series %.3f -> C / A = %.3f, "
              "C - B = %.3f ms (%.3f without the call's set-up: a series of one step takes %.2f ms; %d steps, median of %d rounds)" % (
                  n_sub, A, A_np, B, Cc, Cc / A, Cc - B, steady, C1, STEPS, ROUNDS), flush=True)
if IDEAL:
    bs.close()
if GAINS and not ONE:
    # the kernel trace of one J series (--one-series --gains under rocprofv3 --kernel-trace --stats, a run of its own), where
    # it has been taken: per step and on its own bytes, k_series_solar_gains beside the same trace's k_series_inputs
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_gains_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        kt = {}
        for name, nbytes in (("k_series_solar_gains", gains_bytes["total"]), ("k_series_inputs", inputs_bytes["total"])):
            us = float(rows[name]["AverageNs"]) / 1e3
            kt[name] = dict(calls=int(rows[name]["Calls"]), us_per_step=us, bytes_per_step=nbytes, TB_per_s=nbytes / us / 1e6)
        kt["k_series_apertures_us_per_step"] = float(rows["k_series_apertures"]["AverageNs"]) / 1e3
        kt["rate_over_k_series_inputs"] = kt["k_series_solar_gains"]["TB_per_s"] / kt["k_series_inputs"]["TB_per_s"]
        kt["expectation_rate_at_least_0_95_of_k_series_inputs"] = bool(kt["rate_over_k_series_inputs"] >= 0.95)
        result["kernel_trace_of_one_J_series"] = kt
if AIR and not ONE:
    # the kernel trace of one A series (--one-series --air under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: k_series_air_paths per step beside the same trace's k_series_zone_loads, and the expectation
    # A <= 1.05 (D + k_series_air_paths)
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_air_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_air_paths", "k_series_zone_loads")}
        kt = dict(k_series_air_paths_us_per_step=us["k_series_air_paths"], k_series_zone_loads_us_per_step=us["k_series_zone_loads"],
                  air_paths_over_zone_loads=us["k_series_air_paths"] / us["k_series_zone_loads"], calls=int(rows["k_series_air_paths"]["Calls"]))
        for leg in result["legs"].values():
            leg["expectation_A_at_most_1_05_of_D_plus_the_kernel"] = bool(
                leg["A_series_with_air_paths_ms"] <= 1.05 * (leg["D_series_with_loads_ms"] + us["k_series_air_paths"] * 1e-3))
        result["kernel_trace_of_one_A_series"] = kt
        print("kernel trace: k_series_air_paths %.2f us per step, k_series_zone_loads %.2f (ratio %.2f); A <= 1.05 (D + kernel): %s" % (
            us["k_series_air_paths"], us["k_series_zone_loads"], kt["air_paths_over_zone_loads"],
            {k: v["expectation_A_at_most_1_05_of_D_plus_the_kernel"] for k, v in result["legs"].items()}))
    else:
        print("no kernel trace at %s: the expectation A <= 1.05 (D + k_series_air_paths) is not evaluated" % stats)
if ANISO and not ONE:
    # the kernel trace of one A series (--one-series --aniso under rocprofv3 --kernel-trace --stats, a run of its own), where it has
    # been taken: the anisotropic instantiations of the record's consumers, and the isotropic ones of the warm-up series beside them
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")), os.path.join(here, "series_aniso_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv

        def per_step(path):
            with open(path) as f:
                rows = {r["Name"].split("(")[0].split("::")[-1].replace("void ", ""): r for r in csv.DictReader(f)}
            # (the warm-up's isotropic series is in the same trace: both instantiations, each under its own name)
            return {name: dict(us_per_step=float(r["AverageNs"]) / 1e3, calls=int(r["Calls"])) for name, r in sorted(rows.items())
                    if name.split("<")[0] in ("k_series_blinds", "k_series_sky", "k_series_apertures", "k_series_shading")}
        kt = per_step(stats)
        result["kernel_trace_of_one_A_series"] = kt
        print("kernel trace:", kt)
    else:
        print("no kernel trace at %s" % stats)
if BLINDS and not ANISO and not ONE:
    # the kernel trace of one B series (--one-series --blinds under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: k_series_blinds per step and on its own bytes, beside the same trace's k_series_shading
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_blinds_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_blinds", "k_series_shading", "k_series_sky")}
        nbytes = (BLIND_BYTES["k_series_blinds_per_shade"] + BLIND_BYTES["k_series_blinds_per_blind"]) * S
        result["kernel_trace_of_one_B_series"] = dict(
            k_series_blinds_us_per_step=us["k_series_blinds"], k_series_shading_us_per_step=us["k_series_shading"],
            k_series_sky_us_per_step=us["k_series_sky"], k_series_blinds_bytes_per_step=int(nbytes),
            k_series_blinds_TB_per_s=nbytes / us["k_series_blinds"] / 1e6, calls=int(rows["k_series_blinds"]["Calls"]))
        print("kernel trace: k_series_blinds %.2f us per step (%.2f TB/s on its own bytes), k_series_shading %.2f, k_series_sky %.2f" % (
            us["k_series_blinds"], nbytes / us["k_series_blinds"] / 1e6, us["k_series_shading"], us["k_series_sky"]))
    else:
        print("no kernel trace at %s" % stats)
if SHADES and not BLINDS and not ONE:
    # the kernel trace of one S series (--one-series --shades under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: k_series_shading per step and on its own bytes, beside the same trace's k_series_sky
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_shades_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_shading", "k_series_sky")}
        nbytes = SHADE_BYTES["k_series_shading_per_shade"] * S
        result["kernel_trace_of_one_S_series"] = dict(
            k_series_shading_us_per_step=us["k_series_shading"], k_series_sky_us_per_step=us["k_series_sky"],
            k_series_shading_bytes_per_step=int(nbytes), k_series_shading_TB_per_s=nbytes / us["k_series_shading"] / 1e6,
            calls=int(rows["k_series_shading"]["Calls"]))
        print("kernel trace: k_series_shading %.2f us per step (%.2f TB/s on its own bytes), k_series_sky %.2f" % (
            us["k_series_shading"], nbytes / us["k_series_shading"] / 1e6, us["k_series_sky"]))
    else:
        print("no kernel trace at %s" % stats)
if COMFORT and not ONE:
    # the kernel trace of one C series (--one-series --comfort under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: the two kernels per step, k_series_comfort on its own bytes, beside the same trace's k_series_zone_loads
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_comfort_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_comfort", "k_series_control_T", "k_series_zone_loads")}
        nbytes = COMFORT_BYTES["k_series_comfort_per_entry"] * len(comfort_args["en_sensor"]) + COMFORT_BYTES["k_series_comfort_per_sensor"] * Z
        result["kernel_trace_of_one_C_series"] = dict(
            k_series_comfort_us_per_step=us["k_series_comfort"], k_series_control_T_us_per_step=us["k_series_control_T"],
            k_series_zone_loads_us_per_step=us["k_series_zone_loads"], k_series_comfort_bytes_per_step=int(nbytes),
            k_series_comfort_TB_per_s=nbytes / us["k_series_comfort"] / 1e6, calls=int(rows["k_series_comfort"]["Calls"]))
        print("kernel trace: k_series_comfort %.2f us per step (%.2f TB/s on its own bytes), k_series_control_T %.2f, k_series_zone_loads %.2f" % (
            us["k_series_comfort"], nbytes / us["k_series_comfort"] / 1e6, us["k_series_control_T"], us["k_series_zone_loads"]))
    else:
        print("no kernel trace at %s" % stats)
if AMBIENT and not ONE:
    # the kernel trace of one M series (--one-series --ambient under rocprofv3 --kernel-trace --stats, a run of its own), where
    # it has been taken: k_series_ambient alone
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_ambient_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = float(rows["k_series_ambient"]["AverageNs"]) / 1e3
        result["kernel_trace_of_one_M_series"] = dict(k_series_ambient_us_per_step=us, calls=int(rows["k_series_ambient"]["Calls"]))
        print("kernel trace: k_series_ambient %.2f us per step" % us)
    else:
        print("no kernel trace at %s" % stats)
if NETWORKS and not ONE:
    # the kernel trace of one W series (--one-series --networks under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: k_series_networks per step and per width class, beside the step's other series kernels together
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_networks_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = [r for r in csv.DictReader(f)]
        mine = {r["Name"].split("(")[0].split("::")[-1]: float(r["AverageNs"]) / 1e3 for r in rows if "k_series_networks" in r["Name"]}
        other = sum(float(r["AverageNs"]) / 1e3 for r in rows if "k_series_" in r["Name"] and "k_series_networks" not in r["Name"])
        result["kernel_trace_of_one_W_series"] = dict(k_series_networks_us_per_step=mine, other_series_kernels_us_per_step=other)
        print("kernel trace: k_series_networks %s us per step, the step's other series kernels together %.2f" % (mine, other))
    else:
        result["kernel_trace_of_one_W_series"] = "not taken yet"
        print("no kernel trace at %s" % stats)
if CONTROLLERS and not NETWORKS and not ONE:
    # the kernel trace of one K series (--one-series --controllers under rocprofv3 --kernel-trace --stats, a run of its own), where
    # it has been taken: k_series_controllers per step, beside the same trace's k_series_openings
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_controllers_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_controllers", "k_series_openings")}
        result["kernel_trace_of_one_K_series"] = dict({"%s_us_per_step" % k: v for k, v in us.items()}, calls=int(rows["k_series_controllers"]["Calls"]))
        print("kernel trace: k_series_controllers %.2f us per step, k_series_openings %.2f" % (us["k_series_controllers"], us["k_series_openings"]))
    else:
        result["kernel_trace_of_one_K_series"] = "not taken"
        print("no kernel trace at %s" % stats)
if OPENINGS and not CONTROLLERS and not ONE:
    # the kernel trace of one O series (--one-series --openings under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: k_series_openings per step, beside the same trace's k_series_air_paths
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_openings_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_openings", "k_series_air_paths")}
        result["kernel_trace_of_one_O_series"] = dict({"%s_us_per_step" % k: v for k, v in us.items()}, calls=int(rows["k_series_openings"]["Calls"]))
        print("kernel trace: k_series_openings %.2f us per step, k_series_air_paths %.2f" % (us["k_series_openings"], us["k_series_air_paths"]))
    else:
        result["kernel_trace_of_one_O_series"] = "not taken yet"
        print("no kernel trace at %s" % stats)
if SPECIES and not OPENINGS and not ONE:
    # the kernel trace of one P series (--one-series --species under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: the two kernels per step, beside the same trace's k_series_zone_loads
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_species_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_vents", "k_series_species", "k_series_zone_loads")}
        result["kernel_trace_of_one_P_series"] = dict({"%s_us_per_step" % k: v for k, v in us.items()}, calls=int(rows["k_series_species"]["Calls"]))
        print("kernel trace: k_series_vents %.2f us per step, k_series_species %.2f, k_series_zone_loads %.2f" % (
            us["k_series_vents"], us["k_series_species"], us["k_series_zone_loads"]))
    else:
        result["kernel_trace_of_one_P_series"] = "not taken yet"
        print("no kernel trace at %s" % stats)
if HANDLERS and not SPECIES and not ONE:
    # the kernel trace of one H series (--one-series --handlers under rocprofv3 --kernel-trace --stats, a run of its own), where it
    # has been taken: the two kernels per step, beside the same trace's k_series_zone_loads
    stats = next((a[15:] for a in sys.argv[1:] if a.startswith("--kernel-stats=")),
                 os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_handlers_kernel_stats.csv"))
    if os.path.exists(stats):
        import csv
        with open(stats) as f:
            rows = {r["Name"].split("(")[0].split("::")[-1]: r for r in csv.DictReader(f)}
        us = {name: float(rows[name]["AverageNs"]) / 1e3 for name in ("k_series_handler_units", "k_series_handler_supply", "k_series_zone_loads")}
        result["kernel_trace_of_one_H_series"] = dict({"%s_us_per_step" % k: v for k, v in us.items()}, calls=int(rows["k_series_handler_units"]["Calls"]))
        print("kernel trace: k_series_handler_units %.2f us per step, k_series_handler_supply %.2f, k_series_zone_loads %.2f" % (
            us["k_series_handler_units"], us["k_series_handler_supply"], us["k_series_zone_loads"]))
    else:
        result["kernel_trace_of_one_H_series"] = "not measured"
        print("no kernel trace at %s" % stats)
if not ONE:
    out = OUT or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                              "series_networks.json" if NETWORKS else "series_controllers.json" if CONTROLLERS else "series_openings.json" if OPENINGS else "series_species.json" if SPECIES else "series_handlers.json" if HANDLERS else "series_comfort.json" if COMFORT else "series_aniso.json" if ANISO else "series_blinds.json" if BLINDS else "series_ambient.json" if AMBIENT else "series_radiation.json" if RADIATION else "series_shades.json" if SHADES else "series_air.json" if AIR else "series_gains.json" if GAINS else "series_sky.json" if SKY else "series_ideal.json" if IDEAL else
                              ("series_report.json" if REPORT else ("series_loads.json" if LOADS else "series_march.json")))
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)
