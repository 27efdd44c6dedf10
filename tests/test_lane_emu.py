"""The CPU leg of the lane-local pins: the cases of tests/lane_cases/lane_cases.h on the HOST EMULATOR build (g++ -DDIAL_EMU
-ffp-contract=off) through the gates of tests/lane_ref.py -- the same functions tests/test_gpu_lane_cases.py applies to the two device
builds.  What a gate asks is written at the gate; the figures this build measures are those of the IEEE device build (the two are bit-identical
but for the sign of some zeros) and stand in the table of test_gpu_lane_cases.py.
"""
import numpy as np
import pytest

import lane_lib as L
import lane_ref as R


@pytest.fixture(scope="module")
def emu():
    return L.Emu()


@pytest.mark.parametrize("name", list(R.KINDS))
def test_generic_position_matches_the_fp64_oracle(emu, name):
    rows = R.g1_cases(name)[0]
    R.gate_g1(name, emu.geom(rows), "emulator")


def test_the_edge_pairs_are_edge_contacts():
    """at least 100 of the deliberate edge-edge pairs are edge contacts for the fp64 oracle, and the generator's pairs park and touch"""
    rows, (d64, _p, f64), _ref32, _tol = R.g1_cases("box_box")
    first = 4 * 1000
    assert R.is_edge_contact(rows[first:], d64[first:], f64[first:]).sum() >= 100
    assert (d64[:first:4] > R.PARK).sum() > 100 and (d64[:first:4] < 0).sum() > 100


@pytest.mark.parametrize("gate", list(R.G2_GATES))
def test_degenerate_position_by_geometry(emu, gate):
    R.G2_GATES[gate](emu.geom, "emulator")


def test_polygon_prefill_does_not_reach_the_result(emu):
    rows = R.g1_cases("box_box")[0]
    assert np.array_equal(emu.geom(rows, fill=0), emu.geom(rows, fill=1))


def test_the_exact_capsule_distance_is_the_brute_force_one():
    """segment_box_distance64 (the parked contract's reference for capsules) against test_box_collisions._segment_box_distance"""
    rows = R.g1_cases("capsule_box")[0]
    for row in rows[:24:2]:
        gC, gB = R.row_geoms(row)
        e0, e1 = gC[0] - gC[2][:, 2] * gC[3][1], gC[0] + gC[2][:, 2] * gC[3][1]
        assert abs(R.segment_box_distance64(gC, gB) - R._segment_box_distance(gB[0], gB[2], gB[3], e0, e1)) < 2e-6


def test_segment_helpers_and_make_frame(emu):
    R.gate_segments(emu.seg(R.seg_rows()), "emulator")


def test_keys_are_the_numpy_keys(emu):
    x = R.fkey_inputs()
    R.gate_fkey(emu.key(L.K_FKEY, x[:, None].view(np.int32)), "emulator")


def test_ls_pack(emu):
    R.gate_pack(emu.key(L.K_PACK, R.pack_inputs().view(np.int32)), None, True, "emulator")


def test_bracket_update_per_lane(emu):
    R.gate_update(emu, "emulator")


def test_done_test_forms(emu):
    R.gate_done_test(emu.key(L.K_GATE, R.gate_inputs()), "emulator")


def test_bracket_update_wave_uniform(emu):
    R.gate_uniform(emu, "emulator")


def test_open_and_result(emu):
    R.gate_open_result(emu, "emulator")


def test_axis_angle_to_quat_and_libm_sincos(emu):
    """the emulator's fast_sincos is libm's: this runs the gate's own arithmetic (the device's v_sin_f32 / v_cos_f32 are measured on the GPU)"""
    R.gate_trig(emu.trig(R.trig_rows()), "emulator")
