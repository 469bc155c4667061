"""Bit-for-bit pins of the target build (build_target_map, csrc/voxel_hash.hip) and the candidate-list build
(build_neighbour_lists, csrc/neighbour_lists.hip) against tests/golden/target_build_parent.json: the SHA-256 digests that the
commit before the staged builds computed for the cases of tests/make_golden_target_build.py, through the C ABI.  Equalities: the
oracle comparisons of the other suites allow rounding differences and would not notice a changed build order.  Every digest was
recorded twice at that commit and came out the same both times."""
import pytest

import make_golden_target_build as G

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


def test_full_build_and_candidate_lists(pcm, golden):
    """one point; 257 points in one voxel (across a 256-thread block); a floor across a brick face at negative coordinates; 2000
    points on three faces -- each with the 1 / 7 / 19 / 27 neighbourhood: linearize sums, planes, and the list index (its
    centres are the map order of the index), starts and entries (w = index into the map's point array)"""
    want = golden["full"]
    assert len(want) == 16 and want["full/one_point/nn27"]["lists"] == 27 and want["full/one_voxel_257/nn1"]["lists"] == 1
    assert want["full/scattered_2000/nn27"]["inliers"] > 100
    check(G.compute_full(pcm), want)


def test_incremental_merge(pcm, golden):
    """pcm_set_target, then pcm_target_insert twice: the merged index must give the log and the sums of the parent"""
    want = golden["incremental"]
    assert want["step1"]["points"] == 340 and want["step2"]["points"] == 380
    check(G.compute_incremental(pcm), want)


def test_lru_eviction(pcm, golden):
    """a capacity of 6 voxels and three inserts, the last two overflowing: the compacted log and the batch-hazard count"""
    want = golden["lru"]
    assert want["insert0"]["points"] == 41 and want["insert1"]["points"] < 41 + 16 and want["insert2"]["points"] < want["insert1"]["points"] + 15
    check(G.compute_lru(pcm), want)


def test_map_incremental(pcm, golden):
    """pcm_map_incremental after pcm_obs_model, with the scan in the caller's order and re-ordered on the device"""
    want = golden["map_incremental"]
    assert 0 < want["sort_source0"]["num_added"] < 300 and want["sort_source0"] == want["sort_source1"]
    check(G.compute_map_incremental(pcm), want)


def test_gicp_covariances_and_correspondences(pcm, golden):
    """keep_order, the sub-voxel order and the fine index (covariances come back in input order), and the device-side
    correspondence step"""
    want = golden["gicp"]
    assert want["correspondences"] > 300
    check(G.compute_gicp(pcm), want)


def test_gauss_voxels_leaf_lists_and_voxel_slot_rows(pcm, golden):
    """NDT_D2D linearize (Gauss voxels of both clouds), NDT_OMP derivatives for its four searches (leaf lists), VGICP_CUDA
    linearize (voxel-slot rows)"""
    want = golden["voxel_models"]
    assert len(want) == 6 and want["ndt_d2d"]["inliers"] > 10 and want["vgicp_cuda"]["inliers"] > 100
    assert len({want["ndt_omp/nn%d" % nn]["derivatives"] for nn in (0, 1, 7, 27)}) == 4   # the four searches see different leaves
    check(G.compute_voxel_models(pcm), want)


def test_loam_map(pcm, golden):
    """a small corner / surf target through pcm_loam_coefficients and pcm_loam_neighbours at two poses: the floor-convention,
    kept-order caller.  The maps are sparse, so few features pass the line / plane tests; what pins the build is the neighbour
    indices (caller order) of the features that have any: counts[2] corner and counts[3] surf features"""
    want = golden["loam"]
    assert want["at_truth"]["counts"][2] > 50 and want["at_truth"]["counts"][3] > 300
    check(G.compute_loam(pcm), want)
