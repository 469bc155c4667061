"""Bit-for-bit pins of every VoxelGrid down-sampler (csrc/voxel_grid.h, csrc/voxel_grid.hip) against
tests/golden/voxel_grid_parent.json: the row counts and SHA-256 digests that the commit before the shared implementation
computed for the cases of tests/make_golden_voxel_grid.py.  Equalities: the oracle and numpy comparisons of the other suites
allow 1 ulp and would not notice a changed bit."""
import pytest

import make_golden_voxel_grid as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return G.load()


def check(got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name


def test_voxel_downsample(pcm, golden):
    """one point; 64 and 65 points in one cell (the boundary of the strided lane loop and the butterfly); 300 in one cell plus
    singletons; 2000 points with negative coordinates and non-finite ones, as records of 3, 4, 12 and 16 floats; points on cell
    faces; no finite point at all; the scan of tests/test_preprocess.py at leaf 0.2"""
    G.check_inputs(golden, "downsample")
    want = golden["downsample"]
    assert want["all_non_finite"]["rows"] == 0 and want["one_cell_64"]["rows"] == 1 and want["one_cell_65"]["rows"] == 1
    assert want["one_cell_300_and_5_singletons"]["rows"] == 6
    check(G.compute_downsample(pcm), want)


def test_feature_front_end(pcm, golden):
    """set_input_scan of two scans, the same two as one batch (several frames' segments through one sort), and one frame with
    the mapping leaves at 0 (one cell per element, in order)"""
    G.check_inputs(golden, "features")
    want = golden["features"]
    assert want["single/0/mapping_leaves_0"]["surf"]["rows"] == want["single/0"]["surf_scan"]["rows"] > want["single/0"]["surf"]["rows"]
    check(G.compute_features(pcm), want)


def test_global_map_and_export(pcm, golden):
    G.check_inputs(golden, "global")
    check(G.compute_global(pcm), golden["global"])
