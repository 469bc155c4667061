"""CPU checks of the two batch round schedulers (pointcloud-slam_amd/csrc/batch_schedule.h, compiled with g++ through
tests/batch_schedule_hooks.cpp): the round plan and the launch list of align_batch_impl against a Python restatement of the loop as
it stood before the schedulers were split out (written from that loop, it does not call the header), properties of the launch list
asserted without the restatement, and the lock-step group machine of the batched pclomp NDT registration.  No GPU.

Simulated device: the k-th launch of a running pair writes status byte 1 (active) for k < life[i] and 2 (finished) from k = life[i]
on, so life 1 is a pair that finishes in its first round; a round's bytes exist only for the pairs launched in that round.  With a
device-side window (plans without a host-kept list) a queued pair reports 1 until a finished pair frees its place."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX_LISTED = 128   # kMaxListedPairs (pcm_device.h); pinned by test_max_listed_pairs_constant


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("batch_schedule") / "batch_schedule_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "batch_schedule_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    i, vp = C.c_int, C.c_void_p
    L.bs_plan.argtypes = [i, i, i, i, i, i, vp]
    L.bs_list_new.argtypes = [i, i, i, i, i, i]
    L.bs_list_new.restype = vp
    for f in (L.bs_list_free, L.bs_groups_free):
        f.argtypes = [vp]
        f.restype = None
    for f in (L.bs_list_size, L.bs_list_num_awaited, L.bs_groups_count):
        f.argtypes = [vp]
    L.bs_list_current.argtypes = [vp, vp]
    L.bs_list_awaited.argtypes = [vp, i]
    L.bs_list_advance.argtypes = [vp, vp]
    L.bs_groups_new.argtypes = [i, i, i]
    L.bs_groups_new.restype = vp
    L.bs_group_get.argtypes = [vp, i, vp]
    L.bs_group_try_confirm.argtypes = [vp, i, vp]
    L.bs_group_may_launch.argtypes = [vp, i]
    L.bs_group_launched.argtypes = [vp, i]
    L.bs_group_launched.restype = None
    return L


def test_header_compiles_alone_and_has_no_hip_include():
    hdr = os.path.join(ROOT, "pointcloud-slam_amd", "csrc", "batch_schedule.h")
    assert "#include <hip" not in open(hdr).read() and '#include "' not in open(hdr).read()
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(hdr), "-x", "c++", "-"],
                   input=b'#include "batch_schedule.h"\n', check=True)


def test_max_listed_pairs_constant():
    src = open(os.path.join(ROOT, "pointcloud-slam_amd", "csrc", "pcm_device.h")).read()
    assert "constexpr int kMaxListedPairs = %d;" % K_MAX_LISTED in src


# ---- the restatement: plan and round loop of align_batch_impl before the split ------------------------------------------------
def plan_ref(n, batch_window, max_iterations, is_lm, lm_max_iterations):
    window = min(n, batch_window) if (batch_window > 0 and max_iterations > 0) else n
    per_pair_rounds = max(1, max_iterations) * ((1 + max(1, lm_max_iterations)) if is_lm else 1)
    host_window = window < n and n <= 256 and window <= K_MAX_LISTED
    if host_window:
        max_rounds = ((n + window - 1) // window + 1) * (per_pair_rounds + 1) + 2
    else:
        max_rounds = per_pair_rounds * (n - window + 1) + 1 + 2 * (n - window)
    use_list = (n <= K_MAX_LISTED and window == n) or host_window
    return dict(window=window, per_pair_rounds=per_pair_rounds, host_window=host_window, use_list=use_list, max_rounds=max_rounds)


class Device:
    """The status bytes the step kernel would write (module docstring)."""

    def __init__(self, n, life, plan):
        self.life = list(life)
        self.launches = [0] * n
        self.done = [False] * n
        dev_window = n if plan["host_window"] else plan["window"]   # launch_init_states(..., host_window ? n : window, ...)
        self.running = [i < dev_window for i in range(n)]
        self.next_queued = dev_window
        self.n = n

    def round(self, launched):
        row = np.zeros(self.n, np.uint8)
        freed = 0
        for i in launched:
            if self.done[i]:
                row[i] = 2      # a stale entry exits at once
            elif not self.running[i]:
                row[i] = 1      # queued on the device
            else:
                self.launches[i] += 1
                if self.launches[i] >= self.life[i]:
                    self.done[i] = True
                    freed += 1
                    row[i] = 2
                else:
                    row[i] = 1
        while freed and self.next_queued < self.n:
            self.running[self.next_queued] = True
            self.next_queued += 1
            freed -= 1
        return row


def rounds_ref(n, plan, life):
    """Launched pairs of every round, as the loop before the split chose them."""
    window, host_window, use_list, max_rounds = plan["window"], plan["host_window"], plan["use_list"], plan["max_rounds"]
    dev = Device(n, life, plan)
    flags, out = [], []
    act = list(range(window if host_window else n))
    next_queued = window if host_window else n
    prev_list = []
    for r in range(max_rounds):
        launched = list(act) if use_list else list(range(n))
        out.append(launched)
        flags.append(dev.round(launched))
        this_list = list(act)
        if r >= 1:
            row = flags[r - 1]
            any_active = False
            alive = []
            for i in (prev_list if use_list else range(n)):
                assert row[i] != 0          # the host would wait here for ever
                any_active |= row[i] == 1
                if row[i] == 1 and use_list:
                    alive.append(i)
            if host_window:
                for i in this_list:
                    if i not in prev_list:
                        alive.append(i)
                        any_active = True
                while len(alive) < window and next_queued < n:
                    alive.append(next_queued)
                    next_queued += 1
                    any_active = True
            if not any_active:
                break
            if use_list:
                act = alive
        prev_list = this_list
    return out, dev


def rounds_header(H, n, cfg, plan, life):
    """The same loop driven by LaunchList: what align_batch_impl does now, minus the launches."""
    dev = Device(n, life, plan)
    h = H.bs_list_new(n, *cfg, K_MAX_LISTED)
    buf = np.zeros(256, np.uint8)
    flags, out = [], []
    try:
        for r in range(plan["max_rounds"]):
            if plan["use_list"]:
                m = H.bs_list_current(h, buf.ctypes.data)
                assert m == H.bs_list_size(h)
                launched = [int(x) for x in buf[:m]]
            else:
                assert H.bs_list_size(h) == n
                launched = list(range(n))
            out.append(launched)
            flags.append(dev.round(launched))
            row = flags[r - 1] if r >= 1 else None
            assert (H.bs_list_num_awaited(h) == 0) == (r == 0)
            for k in range(H.bs_list_num_awaited(h)):
                assert row[H.bs_list_awaited(h, k)] != 0   # only bytes that exist are waited for
            if not H.bs_list_advance(h, row.ctypes.data if row is not None else None):
                break
    finally:
        H.bs_list_free(h)
    return out, dev


GRID_N = [1, 2, 7, 64, 128, 129, 256, 257, 700]
BROKE_THE_OLD_BUDGET = (256, (8, 10, 0, 10))   # n, (batch_window, max_iterations, is_lm, lm_max_iterations)


def test_plan_matches_the_restatement_on_the_grid(H):
    out = (C.c_int * 5)()
    cases = 0
    for n in GRID_N:
        for bw in [0, 1, 2, 8, 64, 128, 129, n]:
            for is_lm in (0, 1):
                for it in (0, 1, 10):
                    for lm_it in (0, 10):
                        H.bs_plan(n, bw, it, is_lm, lm_it, K_MAX_LISTED, out)
                        p = plan_ref(n, bw, it, bool(is_lm), lm_it)
                        assert list(out) == [p["window"], p["per_pair_rounds"], int(p["host_window"]), int(p["use_list"]), p["max_rounds"]], (n, bw, is_lm, it, lm_it)
                        cases += 1
    assert cases == 9 * 8 * 2 * 3 * 2


# (n, batch_window): a full list, host windows (even, uneven, one place, the widest), no list, a device-side window
LIST_CONFIGS = [(1, 0), (7, 0), (128, 0), (7, 2), (64, 8), (129, 128), (256, 8), (256, 1), (37, 5), (129, 0), (257, 8), (200, 129)]


def _lives(n, ppr, rng):
    one_straggler = [1] * n
    one_straggler[n // 2] = ppr
    first_round = [ppr] * n
    first_round[0] = 1
    return {"all 1": [1] * n, "all per_pair_rounds": [ppr] * n, "one straggler": one_straggler, "a pair finishing in its first round": first_round,
            "random a": list(rng.integers(1, ppr + 1, n)), "random b": list(rng.integers(1, ppr + 1, n)), "random, mostly short": list(np.minimum(rng.geometric(0.4, n), ppr))}


@pytest.mark.parametrize("n,bw", LIST_CONFIGS)
@pytest.mark.parametrize("solver", [(10, 0, 10), (3, 1, 2)], ids=["GN10", "LM3x2"])
def test_launch_lists_match_the_restatement_round_by_round(H, n, bw, solver):
    cfg = (bw,) + solver
    plan = plan_ref(n, bw, solver[0], bool(solver[1]), solver[2])
    rng = np.random.default_rng(1000 * n + bw)
    for name, life in _lives(n, plan["per_pair_rounds"], rng).items():
        ref, dref = rounds_ref(n, plan, life)
        got, dgot = rounds_header(H, n, cfg, plan, life)
        assert got == ref, name
        assert dgot.done == dref.done, name


def _check_list_properties(n, plan, life, rounds, dev, name):
    if not plan["use_list"]:
        return
    first, last = {}, {}
    for r, lst in enumerate(rounds):
        assert len(lst) <= plan["window"] and len(lst) <= K_MAX_LISTED, name
        assert len(set(lst)) == len(lst) and all(0 <= i < min(n, 256) for i in lst), name
        for i in lst:
            first.setdefault(i, r)
            assert last.get(i, r - 1) == r - 1, (name, "pair %d launched again after a gap" % i)   # consecutive rounds, never again
            last[i] = r
    end = len(rounds) - 1
    for i in first:
        finished_in = first[i] + life[i] - 1
        assert last[i] == min(finished_in + 1, end), (name, i)    # the stale entry: one round after it reported finished


@pytest.mark.parametrize("n,bw", [c for c in LIST_CONFIGS if c[0] <= 256])
def test_launch_list_properties(H, n, bw):
    solver = (10, 0, 10)
    plan = plan_ref(n, bw, *[solver[0], False, solver[2]])
    rng = np.random.default_rng(7 * n + bw)
    for name, life in _lives(n, plan["per_pair_rounds"], rng).items():
        rounds, dev = rounds_header(H, n, (bw,) + solver, plan, life)
        _check_list_properties(n, plan, life, rounds, dev, name)
        assert len(rounds) <= plan["max_rounds"]
        assert all(dev.done), name   # every pair ran to its end within the budget


@pytest.mark.parametrize("n,cfg", [BROKE_THE_OLD_BUDGET, (256, (8, 10, 1, 10)), (255, (8, 10, 0, 10)), (256, (128, 1, 0, 0)), (129, (64, 10, 1, 1)), (9, (8, 10, 0, 10))],
                         ids=["n256_window8_GN10_broke_the_old_budget", "n256_window8_LM10x10", "n255_window8_GN10", "n256_window128_GN1", "n129_window64_LM10x1", "n9_window8_GN10"])
def test_every_pair_running_to_max_iterations_finishes_within_the_budget(H, n, cfg):
    plan = plan_ref(n, cfg[0], cfg[1], bool(cfg[2]), cfg[3])
    assert plan["host_window"]
    life = [plan["per_pair_rounds"]] * n
    rounds, dev = rounds_header(H, n, cfg, plan, life)
    assert all(dev.done) and len(rounds) <= plan["max_rounds"]
    _check_list_properties(n, plan, life, rounds, dev, "all per_pair_rounds")
    ref, _ = rounds_ref(n, plan, life)
    assert rounds == ref


# ---- the lock-step groups of the batched pclomp NDT registration -------------------------------------------------------------------
def _group(H, h, g):
    out = (C.c_int * 5)()
    H.bs_group_get(h, g, out)
    return dict(lo=out[0], hi=out[1], launched=out[2], confirmed=out[3], done=bool(out[4]))


def test_group_ranges_partition_the_objects(H):
    for n in range(1, 34):
        for ng in range(1, min(n, 4) + 1):
            h = H.bs_groups_new(n, ng, 5)
            try:
                assert H.bs_groups_count(h) == ng
                gs = [_group(H, h, g) for g in range(ng)]
            finally:
                H.bs_groups_free(h)
            assert gs[0]["lo"] == 0 and gs[-1]["hi"] == n
            assert all(a["hi"] == b["lo"] for a, b in zip(gs, gs[1:]))
            assert all(g["lo"] < g["hi"] and g["launched"] == 0 and g["confirmed"] == 0 and not g["done"] for g in gs)
            assert max(g["hi"] - g["lo"] for g in gs) - min(g["hi"] - g["lo"] for g in gs) <= 1


def test_pclndt_round_budget(H):
    for it in (0, 1, 30, 64):
        assert H.bs_pclndt_round_budget(it) == (it + 3) * 12 + 2


def _run_groups(H, n, ng, max_rounds, life, lag):
    """Host loop of pclndt_align_batch; a launched round's bytes land 1 + `lag` ticks after its launch.  Returns the groups at the end."""
    h = H.bs_groups_new(n, ng, max_rounds)
    rows = np.zeros((max_rounds + 1, n), np.uint8)      # what has landed
    pending = []                                        # (tick it lands, round, lo, hi)
    ran = np.zeros(n, int)
    try:
        live, tick = ng, 0
        while live > 0:
            tick += 1
            assert tick < 100 * (max_rounds + lag + 2), "the loop does not end"
            for (t, r, lo, hi) in [p for p in pending if p[0] < tick]:
                for i in range(lo, hi):
                    rows[r, i] = 1 if r + 1 < life[i] else 2
            pending = [p for p in pending if p[0] >= tick]
            for g in range(ng):
                G = _group(H, h, g)
                if G["done"]:
                    continue
                if H.bs_group_try_confirm(h, g, rows[G["confirmed"]].ctypes.data):
                    assert rows[G["confirmed"], G["lo"]:G["hi"]].all()      # confirmed only when every byte of the range is there
                    if _group(H, h, g)["done"]:
                        live -= 1
                        continue
                if H.bs_group_may_launch(h, g):
                    G = _group(H, h, g)
                    assert G["launched"] - G["confirmed"] < 2 and G["launched"] < max_rounds
                    pending.append((tick + lag, G["launched"], G["lo"], G["hi"]))
                    ran[G["lo"]:G["hi"]] += 1
                    H.bs_group_launched(h, g)
                G = _group(H, h, g)
                assert 0 <= G["launched"] - G["confirmed"] <= 2      # never more than two unconfirmed rounds
        return [_group(H, h, g) for g in range(ng)], ran
    finally:
        H.bs_groups_free(h)


@pytest.mark.parametrize("lag", [0, 1, 3])
def test_groups_stop_one_round_after_their_last_object_and_at_the_budget(H, lag):
    rng = np.random.default_rng(lag)
    for n, ng in [(1, 1), (5, 2), (8, 4), (16, 2), (33, 3), (33, 4)]:
        max_rounds = 40
        life = rng.integers(1, 30, n)
        life[n - 1] = 1000                       # the last group never finishes: it stops at the budget
        gs, ran = _run_groups(H, n, ng, max_rounds, life, lag)
        for G in gs:
            assert G["done"]
            longest = int(life[G["lo"]:G["hi"]].max())
            if longest > max_rounds:
                assert G["confirmed"] == max_rounds and G["launched"] == max_rounds
            else:
                assert G["confirmed"] == longest                                   # the round in which its last object finished
                assert G["launched"] == (longest + 1 if lag else longest)          # seen one round late: one more was in flight
            assert (ran[G["lo"]:G["hi"]] == G["launched"]).all()
