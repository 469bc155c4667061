#!/usr/bin/env python
"""Measures the bounds tests/test_gpu_lio_propagate.py holds pcm_lio_propagate to, on the CPU, from the numpy restatement alone
(tests/lio_predict_ref.py): each test frame is restated once as is and 20 times with every sin / cos / sqrt / atan result moved by
+-1 ulp at random; the worst relative difference per output group (state, P, poses) is printed as the MEASURED table of the test.
No GPU, no library."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import lio_predict_case as case  # noqa: E402
import lio_predict_ref as PR  # noqa: E402


def main():
    import test_gpu_lio_propagate as T
    print("MEASURED = {")
    for key in T.CASES:
        c = T.make_case(key)
        w = PR.libm_sensitivity(lambda: case.groups(case.restate(c)), draws=20, seed=1)
        print("    %r: dict(state=%.1e, P=%.1e, poses=%.1e)," % (key, w["state"], w["P"], w["poses"]))
    c1, c2 = T.two_frames()

    def both():
        a = case.restate(c1)
        b = case.restate(dict(c2, s=a["s"], x=a["x"], P=a["P"]))
        return case.groups(b)
    w = PR.libm_sensitivity(both, draws=20, seed=1)
    print("    %r: dict(state=%.1e, P=%.1e, poses=%.1e)," % ("two_calls", w["state"], w["P"], w["poses"]))
    print("}")


if __name__ == "__main__":
    main()
