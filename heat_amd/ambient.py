"""Ambient-side temperatures of a series on the host (include/heat_amd.h, heat_ambient_drive): the rule the device applies to
every driven side at every step, in numpy. No device, no library.

apply() IS the contract's rule, line for line — every product and sum one rounded f64 operation in the header's order (numpy
never fuses a multiply-add) — and so the reference of the tests: a host that downloads the zone temperatures before every
heat_batch_march_ex call, applies it and hands the values to heat_batch_set_ambient gets the bits of
heat_batch_march_series_ambient.
The reference has no counterpart: its boundaries are fixed when the model is built."""
import numpy as np


def b_factor(b):
    """mix = 1 - b for the temperature-reduction factor b of EN ISO 13789 / EN 12831: an unheated space sits at
    T_u = T_out + (1 - b) * (T_zone - T_out). b = 1: outside; b = 0: the zone's own temperature."""
    return 1.0 - np.asarray(b, dtype=np.float64)


def apply(drive, row, zone_T):
    """The ambient temperature of every driven side in one step: [n_sides].
    drive   a dict of make_ambient's arguments: chan, and optionally gain, offset, mix_zone, mix (surface, side and
            sum_temperature are not read)
    row     [n_channels] the step's row of the channel table
    zone_T  [n_zones] the zone temperatures when the step starts (not read without a mix_zone >= 0)
        v = row[chan];  v = gain * v;  v = v + offset;  where mix_zone >= 0:  d = T[mix_zone] - v;  m = mix * d;  v = v + m"""
    row = np.asarray(row, dtype=np.float64)
    chan = np.asarray(drive["chan"], dtype=np.int64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = row[chan]
        if drive.get("gain") is not None:
            v = np.asarray(drive["gain"], dtype=np.float64) * v
        if drive.get("offset") is not None:
            v = v + np.asarray(drive["offset"], dtype=np.float64)
        if drive.get("mix_zone") is not None:
            zone = np.asarray(drive["mix_zone"], dtype=np.int64).reshape(-1)
            on = zone >= 0
            if on.any():
                d = np.asarray(zone_T, dtype=np.float64)[zone[on]] - v[on]
                m = np.asarray(drive["mix"], dtype=np.float64)[on] * d
                v = v.copy()
                v[on] = v[on] + m
    return v
