"""Bit-for-bit pins of the jueying_lio entry points (csrc/lio_api.hip) against tests/golden/lio_api_parent.json: the SHA-256
digests that the commit before they left csrc/pcm_api.hip computed for the cases of tests/make_golden_lio_api.py, through the C
ABI.  Equalities: the oracle comparisons of the other suites allow rounding differences and would not notice a changed pose
expression, sort guess or launch order.  The file was recorded with the library built from that commit (PCM_AMD_LIBRARY), twice,
and both recordings were identical.

The one intended difference to that commit is pinned at the end: whatever replaces the source also drops the planes of the last
matching call, so pcm_obs_model(rematch = 0) after pcm_swap_source_and_target is refused instead of reading the old scan's planes."""
import pytest

import make_golden_lio_api as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = G.load()
    G.check_inputs(g)
    return g


def check(got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name


def test_obs_model(pcm, golden):
    """257 points (two 256-point tiles) and 16, sort_source 0 / 1, with and without the reference semantics, on the tile kernel and
    on following lists: the sums, planes, members and search-path counters of a matching call and of a rematch = 0 call after it"""
    want = golden["obs_model"]
    assert len(want) == 16
    for path in ("tiles", "lists"):
        case = want["n257/sort1/ref0/" + path]
        assert case["match"]["n_eff"] > 100 and case["update"]["n_eff"] > 100 and len(case["match"]["HTH"]) == 64
    assert want["n257/sort1/ref0/lists"]["match"]["search_path"] == [1, 0] and want["n257/sort1/ref0/tiles"]["match"]["search_path"] == [0, 1]
    assert want["n257/sort0/ref0/tiles"]["update"]["search_path"] == [0, 1]      # a rematch = 0 call searches nothing
    assert want["n16/sort0/ref1/tiles"]["match"]["n_eff"] >= 1
    check(G.compute_obs_model(pcm), want)


def test_lio_update(pcm, golden):
    """max_iter 1 and 4 on tiles and on lists: x, P, the result and the trace of every executed ObsModel call"""
    want = golden["lio_update"]
    assert len(want) == 4
    for name, case in want.items():
        iterations, rematches, valid_calls, t, n_eff_last, status = case["result"]
        assert status == 0 and 1 <= iterations <= int(name[4]) + 1 and rematches >= 1 and valid_calls >= 1 and n_eff_last > 100 and len(case["trace"]) == iterations
    assert want["iter4/tiles"]["result"][0] > want["iter1/tiles"]["result"][0]
    check(G.compute_lio_update(pcm), want)


def test_map_incremental(pcm, golden):
    """after pcm_obs_model and after pcm_lio_update, on tiles and on lists, and on lists behind a pcm_target_insert the lists have
    followed (the generation guard of the neighbours decides)"""
    want = golden["map_incremental"]
    assert len(want) == 5
    guarded = want["after_obs_and_insert/lists"]
    for name, case in want.items():
        assert case is guarded or 0 < case["num_added"] < 257, name
    # the neighbours index list entries that moved: MapIncremental runs without them and, like the reference without
    # nearest points, adds every scan point -- a guard that let them through would have filtered as in after_obs/lists
    assert guarded["num_added"] == 257 and guarded["points"] == 3000 + 40 + 257
    check(G.compute_map_incremental(pcm), want)


def _frames_not_degenerate(want):
    assert len(want) == 8
    for name, case in want.items():
        assert (100 < case["n_scan"] < 600) if name.startswith("leaf0.5") else (300 < case["n_scan"] <= 600)
    assert want["leaf0.5/poses0/host"]["n_scan"] < want["leaf0/poses0/host"]["n_scan"]
    assert want["leaf0/poses3/host"]["body"] != want["leaf0/poses0/host"]["body"]         # the compensation moved points
    assert want["leaf0/poses3/host"] == want["leaf0/poses3/device"]


def test_frame_begin(pcm, golden):
    """a 600-record Livox message: leaf 0 / 0.5, no poses / three, from host and from device memory"""
    _frames_not_degenerate(golden["frame_begin"])
    check(G.compute_frame_begin(pcm), golden["frame_begin"])


def test_frame_begin_cloud(pcm, golden):
    """a 600-point RoboSense cloud with the same variations"""
    _frames_not_degenerate(golden["frame_begin_cloud"])
    check(G.compute_frame_begin_cloud(pcm), golden["frame_begin_cloud"])


def test_undistort(pcm, golden):
    want = golden["undistort"]
    assert want["host"] == want["device"] and want["host"] != G.sha(G.inputs()["records"][0])
    check(G.compute_undistort(pcm), want)


REFUSAL = "pcm_obs_model(rematch=0) before any matching call"


def _refused_on_the_host(pcm, g):
    before = (g.stats(), g.lio_search_path())
    with pytest.raises(pcm.PcmError) as e:
        g.obs_model(*G._st(1), False, False)
    assert e.value.code == pcm.capi.PCM_ERR_INVALID_ARGUMENT and REFUSAL in str(e.value)
    assert (g.stats(), g.lio_search_path()) == before       # no build, no launch, nothing counted


def test_obs_model_without_rematch_is_refused_after_the_source_was_replaced(pcm):
    """sort_source = 0, so the only thing between a rematch = 0 call and the old scan's planes is lio_planes_valid"""
    submap, scan, _ = G.inputs()["scene"]
    g = G._reg(pcm, scan, sort_source=0)
    g.obs_model(*G._st(0), False, True)
    g.obs_model(*G._st(1), False, False)           # served: the planes are this scan's
    g.swap_source_and_target()
    _refused_on_the_host(pcm, g)
    g = G._reg(pcm, scan, sort_source=0)
    g.obs_model(*G._st(0), False, True)
    g.clear_source()
    g.set_input_source(scan[:200])
    _refused_on_the_host(pcm, g)
