"""How a batch call feeds its workers: the headline shape of bench.py (6144 pairs of 1242 x 375, the four urban crops
tiled, six workers, 32 pairs per launch) through svh_elas_process_batch_device, with svh_elas_feed_stats read after
every call.

    python tools/gpu_feed.py [--feed 7,0] [--calls 8] [--pairs 6144] [--out profiles/feed_counters.jsonl]

For each value of SVH_FEED in --feed (a bit set: 1 = lane parity set at acquisition, 2 = groups in fixed shares,
4 = lanes refilled in strict alternation; 7 = the engine before the group feed, 0 = the default) the lanes are
dropped (svh_elas_trim) and --calls calls are made.  One JSON line per call:
    pairs_per_s   of that call (host clock around the call, which ends in the library's own waits)
    lanes, streams   what the device's lane pool holds after the call, streams per priority class
    taken         groups every worker took
    finish_ms     when every worker's last group finished, from the start of the call
    spread_pct    (latest - earliest finish) / duration of the call: how long the quickest worker's queues stood empty
    out_of_turn   groups that went to the lane filled last because it was free first (this call)
and one summary line per value.  The first call of a value sizes the lanes' buffers and is left out of the summary."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1242, 375
URBAN = ["urban%d_1242x375" % i for i in (1, 2, 3, 4)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--feed", default="7,0")
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=6144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_counters.jsonl"))
    a = ap.parse_args()
    import helpers as Hh
    import svhip as S
    assert S.device_count() > 0, "no HIP device: nothing is measured without one"
    hip = C.CDLL("libamdhip64.so")
    B = a.pairs
    pairs = [Hh.golden_pair(n) for n in URBAN]
    bufs = {}
    for k, nbytes in (("I1", B * W * H), ("I2", B * W * H), ("D1", B * W * H * 4), ("D2", B * W * H * 4)):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        bufs[k] = p
    for side, k in ((0, "I1"), (1, "I2")):
        for i in range(B):
            img = np.ascontiguousarray(pairs[i % 4][side])
            assert hip.hipMemcpy(C.c_void_p(bufs[k].value + i * W * H), C.c_void_p(img.ctypes.data), C.c_size_t(W * H), 1) == 0
    e = S.Elas(Hh.robotics())
    dims = (C.c_int32 * 3)(W, H, W)
    st = (C.c_int32 * B)()
    lines = []
    for bits in [int(x) for x in a.feed.split(",")]:
        os.environ["SVH_FEED"] = str(bits)
        S.trim()
        spreads, rates = [], []
        turn0 = S.feed_stats()["out_of_turn"]
        for call in range(a.calls):
            t0 = time.perf_counter()
            rc = S.lib().svh_elas_process_batch_device(e._h, B, bufs["I1"], bufs["I2"], W * H, bufs["D1"], bufs["D2"],
                                                       W * H * 4, dims, st)
            dt = time.perf_counter() - t0
            assert rc == 0 and not any(st), (rc, S.last_error())
            fs = S.feed_stats()
            fin = fs["finish_us"]
            spread = 100.0 * (max(fin) - min(fin)) / max(fs["call_us"], 1)
            line = {"tool": "gpu_feed", "SVH_FEED": bits, "call": call, "pairs_per_s": round(B / dt, 1),
                    "call_ms": round(fs["call_us"] / 1e3, 2), "lanes": fs["lanes"], "streams": fs["streams"],
                    "taken": fs["taken"], "finish_ms": [round(us / 1e3, 2) for us in fin],
                    "spread_pct": round(spread, 2), "out_of_turn": fs["out_of_turn"] - turn0}
            turn0 = fs["out_of_turn"]
            if call:
                spreads.append(spread)
                rates.append(B / dt)
            lines.append(line)
            print(json.dumps(line), flush=True)
        if rates:
            line = {"tool": "gpu_feed", "SVH_FEED": bits, "summary_of_calls": len(rates),
                    "pairs_per_s_median": round(float(np.median(rates)), 1),
                    "spread_pct_median": round(float(np.median(spreads)), 2),
                    "spread_pct_min": round(min(spreads), 2), "spread_pct_max": round(max(spreads), 2),
                    "queue_plan": S.queue_plan(), "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "")}
            lines.append(line)
            print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    for p in bufs.values():
        hip.hipFree(p)


if __name__ == "__main__":
    main()
