"""Generate tests/golden/vo_mono_edges.npz: more estimate-only cases of VisualOdometryMono, in the est_<name>_* layout
of vo_mono.npz (make_goldens_mono.py).  RUNS ONLY IN THE BUILD CONTAINER.

The cases of vo_mono.npz have N in {9, 10, 12, 50, 200, 300, 350, 2000, 5000} and 500 or 2000 iterations.  These have
the sizes at which the kernels of vo_mono_kernels.hip change rounds (mono_ref.edge_cases):
  * n<N>       N in EDGE_N with the demo's parameters;
  * iters<I>   ransac_iters in EDGE_ITERS at N = 300.  With 0 iterations the reference runs without a fault: it finds
               no inlier and returns false;
  * tie_*      noiseless inliers, half the matches random pairs and a loose inlier_threshold: several hypotheses reach
               the largest count, and one of them later than the first sits in a lower lane of k_mono_select
               (mono_ref.tie_of).  tie_high has its first maximum beyond hypothesis 255.
The matches themselves are stored: nothing has to be drawn again to use the fixture.

    python tests/golden/make_goldens_mono_edges.py            write the fixture
    python tests/golden/make_goldens_mono_edges.py --search   print seeds whose votes meet mono_ref.tie_of
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mono_ref as R  # noqa: E402

LIMIT = 1024 * 1024


def search(exe, tmp):
    for n, thr in ((200, 1e-4), (120, 1e-3)):
        pvec = R.param_vector(dict(R.DEMO, inlier_threshold=thr, motion_threshold=1e6))
        for seed in range(100, 140):
            m = R.synth_scene(n, seed, ground=0.3, noise=0.0, outliers=0.5)
            ok, inl, T, votes = R.run_estimate(exe, tmp, pvec, m)
            if R.tie_of(votes):
                print("N", n, "threshold", thr, "seed", seed, "ok", ok, "(h0, h1, count, ties)", R.tie_of(votes))


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        if "--search" in sys.argv:
            return search(exe, tmp)
        cases = R.edge_cases()
        out["est_names"] = np.array([c[0] for c in cases])
        for name, pvec, m in cases:
            ok, inl, T, votes = R.run_estimate(exe, tmp, pvec, m)
            assert len(votes) == int(pvec[5]) and len(m) >= 10, name
            out["est_%s_params" % name] = pvec
            out["est_%s_matches" % name] = m
            out["est_%s_ok" % name] = np.array(ok, np.int32)
            out["est_%s_inliers" % name] = inl
            out["est_%s_motion" % name] = T
            out["est_%s_votes" % name] = votes
            print(name, "N", len(m), "ok", ok, "inliers", len(inl), "votes", len(votes),
                  "max", int(votes.max()) if len(votes) else None, "tie", R.tie_of(votes))
        ties = [R.tie_of(out["est_%s_votes" % t[0]]) for t in R.EDGE_TIES]
        assert all(ties) and any(t[0] >= 256 for t in ties) and any(t[0] < 256 for t in ties), ties
    np.savez_compressed(R.EDGE_GOLDEN, **out)
    size = os.path.getsize(R.EDGE_GOLDEN)
    print("vo_mono_edges.npz", size // 1024, "KiB")
    if size > LIMIT:
        raise SystemExit("vo_mono_edges.npz is larger than %d bytes" % LIMIT)


if __name__ == "__main__":
    main()
