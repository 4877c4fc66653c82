"""Writes tests/golden/histnorm.npz: what the reference's StereoImage::histogramNormalization
(stereomapper/stereoimage.cpp, compiled unchanged over a QObject stand-in) computes for the cases of
tests/histnorm_ref.py.  Needs the reference's sources (REF, default /root/reference).  Recorded results only: per case
the map as the output shows it (histnorm_ref.observed_map) and the output image (small cases) or its SHA-256; the
inputs are committed crops or closed formulas (histnorm_ref.cases).

    python tests/golden/make_goldens_histnorm.py [--check]     (--check: compare with the committed file, write nothing)

Every case must take the branch it is there for IN THE REFERENCE'S OWN OUTPUT; the assertions below stop the script
otherwise, so that no case passes by missing its subject."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import histnorm_ref as R  # noqa: E402


def check_branch(name, before, after, m):
    if name == "flat_1392x512":
        assert (after == 1).all(), (name, np.unique(after))             # 257 wrapped through the byte
    elif name == "flat_1242x375":
        assert (after == 254).all(), (name, np.unique(after))           # the chain ends below 1
    elif name == "two_1392x512":
        assert m[10] == 84 and m[200] == 255 and sorted(np.unique(after)) == [84, 255], (name, m[10], m[200])
    elif name.startswith("ramp"):
        assert len(np.unique(before)) == 256, name
    elif name.startswith("boundary"):
        assert (R.counts_of(before)[:9] > 0).all(), name                # at least three breakpoints are in it
    elif name == "one_1x1":
        assert after[0, 0] == 255, name
    else:
        assert len(np.unique(before)) > 8, name


def main():
    check_only = "--check" in sys.argv
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name, img, step, keep in R.cases():
            after, = R.run_reference(exe, tmp, [(img, step)])
            m = R.observed_map(img, after)
            check_branch(name, img, after, m)
            out[name + "_map"] = m
            out[name + ("_img" if keep else "_sha")] = after if keep else R.sha(after)
            names.append(name)
            print("%-22s %5dx%-5d levels %3d map[min..max] %3d..%3d" % (name, img.shape[1], img.shape[0],
                                                                        len(np.unique(img)), m[img.min()], m[img.max()]))
    out["case_names"] = np.array(names)
    if check_only:
        Z = R.load_golden()
        assert sorted(Z) == sorted(out), "the fixture has other arrays"
        for k in out:
            assert np.asarray(out[k]).tobytes() == Z[k].tobytes() and np.asarray(out[k]).dtype == Z[k].dtype, k
        print("histnorm.npz: every array is content-equal to what the reference gives today")
        return
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote %s: %d bytes" % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
