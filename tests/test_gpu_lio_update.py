"""GPU parity of pcm_lio_update -- jueying_lio's iterated Kalman update with every ObsModel call and the 23 x 23 algebra on the device --
against the numpy restatement of the reference (tests/lio_iekf_ref.py) driven by the oracle's ObsModel.

Tolerances (max |a - b| / max |b| per compared array) are 10 x the worst difference measured between the device and the restatement
on the input of the test; the margin covers LU pivot-order and device-libm differences accumulated over <= 5 iterations.
  frame of tests 1, 2, 6 (8 000 points, guess = truth + (0.15 m, 2 deg)):  measured 2.8e-11 -> FRAME_TOL 2.8e-10
  16-point scan, device information form vs restatement dense form:      measured 3.2e-9  -> FEW_TOL 3.2e-8"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_iekf_ref as ref  # noqa: E402
import lio_update_case as case  # noqa: E402
from helpers import HB_RTOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED_FRAME = 2.8e-11    # ext 0: 1.1e-13, ext 1: 2.8e-11, host-driven loop: 6.1e-14
FRAME_TOL = 10 * MEASURED_FRAME
MEASURED_FEW = 3.2e-9
FEW_TOL = 10 * MEASURED_FEW


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def frame():
    return case.frame()


@pytest.fixture(scope="module")
def restated(frame):
    """The restatement on the oracle's ObsModel, extrinsic_est_en 0 and 1: computed once."""
    from oracle import Oracle
    p, x0, P0 = frame
    out = {}
    for ext in (0, 1):
        o = Oracle("P2PLANE", "GN", **case.KW)
        o.set_input_target(p.submap); o.set_input_source(p.scan)
        out[ext] = ref.update(x0, P0, ref.oracle_callback(o, p.scan[:, :3], ext), max_iter=4)
    return out


def _reg(pcm, p, scan=None, **kw):
    g = pcm.P2PlaneRegistration(0, **case.KW, **kw)
    g.set_input_target(p.submap); g.set_input_source(p.scan if scan is None else scan)
    return g


def _compare(g, r, want):
    """Trace, state and P of a device update against a restatement run -> worst relative difference of dx_, state, P."""
    assert (r.iterations, r.rematches, r.valid_calls, r.t) == (want["iterations"], want["rematches"], want["valid_calls"], want["t"])
    worst = 0.0
    for k, tr in enumerate(want["trace"]):
        got = g.lio_update_trace(k)
        assert got["converge"] == tr["converge"] and got["n_eff"] == tr["n_eff"], (k, got["converge"], got["n_eff"], tr["converge"], tr["n_eff"])
        if tr["n_eff"]:
            assert rel_err(got["HTH"], tr["HTH"]) < HB_RTOL and rel_err(got["HTh"], tr["HTh"]) < HB_RTOL
        worst = max(worst, _rel(ref.state_to_vec(got["x"]), ref.state_to_vec(tr["x"])))
        if tr["dx_"].any():
            worst = max(worst, _rel(got["dx_"], tr["dx_"]))
    worst = max(worst, _rel(ref.state_to_vec(r.x), ref.state_to_vec(want["x"])), _rel(r.P, want["P"]))
    return worst


@pytest.mark.parametrize("ext", [0, 1])
def test_trace_matches_restatement(pcm, frame, restated, ext):
    """Every ObsModel call of the device loop has the restatement's converge flag and n_eff, its sums within HB_RTOL; dx_, the final
    state and the final P within FRAME_TOL.  The restatement itself takes calls with converge = false, the forced re-match at
    i == max_iter - 2 and the run-to-max_iter exit on this frame (checked here)."""
    p, x0, P0 = frame
    want = restated[ext]
    flags = [t["converge"] for t in want["trace"]]
    assert False in flags and want["iterations"] == 5 and flags[-1] and want["t"] == 0     # converge = false calls, forced re-match, exit at max_iter
    g = _reg(pcm, p)
    r = g.lio_update(x0, P0, extrinsic_est_en=bool(ext))
    assert r.status == 0
    worst = _compare(g, r, want)
    print("frame ext=%d worst rel %.3e" % (ext, worst))
    assert worst <= FRAME_TOL
    e0, e1 = case.pose_error(x0, p.T_gt), case.pose_error(r.x, p.T_gt)
    assert e1[0] < e0[0] and e1[1] < e0[1]                                                  # sanity: closer to the truth than the guess
    assert np.abs(r.P - r.P.T).max() <= FRAME_TOL * np.abs(r.P).max()


def _host_loop(g, x0, P0, ext, **kw):
    """The loop as a caller writes it today: the restatement on the host, pcm_obs_model for every ObsModel call."""
    def h(x, converge):
        HTH, HTh, n_eff, s2, valid = g.obs_model(x["rot"], x["pos"], x["off_R"], x["off_T"], bool(ext), converge)
        return dict(valid=valid, HTH=HTH, HTh=HTh, n_eff=n_eff, sum_h2=s2)
    return ref.update(x0, P0, h, dense=False, **kw)


def test_equals_host_driven_loop(pcm, frame):
    """The same frame through pcm_obs_model with the restatement between the calls: identical (re-match, n_eff) sequence, final state
    and P within FRAME_TOL."""
    p, x0, P0 = frame
    g1, g2 = _reg(pcm, p), _reg(pcm, p)
    r = g1.lio_update(x0, P0)
    want = _host_loop(g2, x0, P0, 0, max_iter=4)
    seq = [(g1.lio_update_trace(k)["converge"], g1.lio_update_trace(k)["n_eff"]) for k in range(r.iterations)]
    assert seq == [(t["converge"], t["n_eff"]) for t in want["trace"]]
    worst = _compare(g1, r, want)
    print("host loop worst rel %.3e" % worst)
    assert worst <= FRAME_TOL


def test_few_effective_points(pcm, frame):
    """16 points of the scan: 1 <= n_eff < 23, where the reference takes the dense gain (esekfom.hpp:1618-1648) and the device the
    information form -- the documented deviation.  Device vs restatement (dense, rows rebuilt from the oracle's planes and checked against
    its HTH) within FEW_TOL."""
    from oracle import Oracle
    p, x0, P0 = frame
    scan = case.few_points(p)
    o = Oracle("P2PLANE", "GN", **case.KW)
    o.set_input_target(p.submap); o.set_input_source(scan)
    cb = ref.oracle_callback(o, scan[:, :3], 0, with_rows=True)
    seen = []

    def h(x, converge):
        m = cb(x, converge)
        seen.append(m)
        assert len(m["h"]) == m["n_eff"] and rel_err(m["h_x"].T @ m["h_x"], m["HTH"]) < 1e-12 and rel_err(m["h_x"].T @ m["h"], m["HTh"]) < 1e-12
        return m
    want = ref.update(x0, P0, h, max_iter=4)
    assert all(1 <= m["n_eff"] < 23 for m in seen)                                           # the dense branch, every call
    g = _reg(pcm, p, scan=scan)
    r = g.lio_update(x0, P0)
    worst = _compare(g, r, want)
    print("few points worst rel %.3e" % worst)
    assert worst <= FEW_TOL


def test_no_effective_points(pcm, frame):
    """A scan 1e4 m away: every call is invalid, the loop runs all max_iter + 1 calls, state and P come back bit for bit."""
    p, x0, P0 = frame
    far = np.full((64, 3), 1.0e4, np.float32)
    g = _reg(pcm, p, scan=far)
    Pd = P0 + 1e-7 * np.arange(529).reshape(23, 23)          # not symmetric, not diagonal: nothing may touch it
    r = g.lio_update(x0, Pd, max_iter=3)
    assert (r.valid_calls, r.iterations, r.rematches, r.t, r.n_eff_last) == (0, 4, 4, 0, 0)
    assert np.array_equal(ref.state_to_vec(r.x), ref.state_to_vec(x0)) and np.array_equal(r.P, Pd)


def test_frame_api_map_equals_host_driven_loop(pcm, synth):
    """lio_frame_begin -> lio_update -> lio_frame_end over three frames with the sliding map: the map equals the one the host-driven
    loop (pcm_obs_model + restatement) leaves."""
    scene = synth.scene_for_points(1234, 60000, 8.0)
    submap = synth.sample_submap(scene, 60000, 4321)
    T = synth.sensor_pose(scene, 77)
    g1 = pcm.P2PlaneRegistration(0, **case.KW); g2 = pcm.P2PlaneRegistration(0, **case.KW)
    g1.set_input_target(submap); g2.set_input_target(submap)
    P0 = np.diag(ref.INIT_P_DIAG)
    kw = dict(num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.5)
    for f in range(3):
        Tf = T.copy(); Tf[:3, 3] += Tf[:3, 0] * 0.6 * f
        sc, ex = synth.livox_scan(scene, Tf, 6000, 555 + f, point_filter_num=1)
        msg = synth.custom_msg(sc, ex)
        x0 = case.filter_state(case.perturb(Tf, 0.05, 0.5))
        st0 = (x0["rot"], x0["pos"], x0["off_R"], x0["off_T"])
        n1 = g1.lio_frame_begin(msg, None, *st0, **kw); n2 = g2.lio_frame_begin(msg, None, *st0, **kw)
        assert n1 == n2 > 500
        r = g1.lio_update(x0, P0)
        want = _host_loop(g2, x0, P0, 0, max_iter=4)
        assert r.iterations == want["iterations"] and r.valid_calls == want["valid_calls"] >= 2
        a1 = g1.lio_frame_end(r.x["rot"], r.x["pos"], r.x["off_R"], r.x["off_T"], 0.5, True)
        a2 = g2.lio_frame_end(want["x"]["rot"], want["x"]["pos"], want["x"]["off_R"], want["x"]["off_T"], 0.5, True)
        assert a1 == a2 > 0
        assert np.array_equal(g1.get_target(), g2.get_target())


def test_run_to_run_identity(pcm, frame):
    p, x0, P0 = frame
    runs = []
    for _ in range(2):
        g = _reg(pcm, p)
        r = g.lio_update(x0, P0, extrinsic_est_en=True)
        runs.append((ref.state_to_vec(r.x), r.P, np.array([g.lio_update_trace(k)["dx_"] for k in range(r.iterations)]), r.iterations, r.t))
    a, b = runs
    assert a[3:] == b[3:]
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


def test_errors(pcm, frame):
    """A non-P2PLANE context, no source, max_iter < 1, a non-finite P: a status and a readable message, no fault."""
    p, x0, P0 = frame
    g = pcm.GicpRegistration(0)
    g.set_input_target(p.submap[:2000]); g.set_input_source(p.scan[:500])
    with pytest.raises(pcm.PcmError, match="P2PLANE"):
        g.lio_update(x0, P0)
    g = pcm.P2PlaneRegistration(0, **case.KW)
    g.set_input_target(p.submap)
    with pytest.raises(pcm.PcmError) as e:
        g.lio_update(x0, P0)
    assert len(str(e.value)) > 20
    g.set_input_source(p.scan)
    with pytest.raises(pcm.PcmError, match="max_iter"):
        g.lio_update(x0, P0, max_iter=0)
    bad = P0.copy(); bad[3, 4] = np.nan
    with pytest.raises(pcm.PcmError, match="finite"):
        g.lio_update(x0, bad)
    with pytest.raises(pcm.PcmError):
        g.lio_update_trace(0)                     # no update has run on this object
    r = g.lio_update(x0, P0)                      # and the object still works
    assert r.status == 0 and r.valid_calls >= 2
