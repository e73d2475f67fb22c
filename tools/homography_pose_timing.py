"""The pose-from-planes entries beside the sequential restatement, and the existing plane entries of two BUILDS of the library.

  python tools/homography_pose_timing.py [--reps 30] [--out profiles/homography_pose_timing.txt] [--parent-lib PATH] [--ab-reps 5]

One command measures everything (wall time around calls that end in a synchronise; every shape is warmed up first; every figure is
printed as median [min .. max] over its repetitions):
  * mlpl_homography_alignment_dev alone (planted labels) on the 900-point three-plane scene p3_n900 and on the 4100-point scene
    p2_n4100 of tests/homography_pose_scenes.py, beside the restatement tests/cpp/homography_align_oracle.cpp on one CPU thread;
  * mlpl_pose_homographies_dev (plane search included, fresh streams per call) on full_three, beside the composition of the two
    restatements;
  * 512 problems like full_three (seeds 1 ... 512, fresh streams per problem): one mlpl_pose_homographies_batch_dev call against the loop of
    512 mlpl_pose_homographies_dev calls on one context, alternating, five repetitions, results compared by bytes as they are timed;
  * with --parent-lib: mlpl_homography_arrsac_dev on n5000_half and mlpl_mult_homographies_dev on three for the parent's build and this
    one (the child mode of tools/homography_batch_timing.py, a fresh process per repetition, alternating): the existing entries must
    not pay for the larger kernel table."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

FRESH = (0xFFFFFFFF, 0xFFFFFFFF)


def fmt(ts):
    return f"median {np.median(ts):.3f} ms [min {min(ts):.3f} .. max {max(ts):.3f}] over {len(ts)}"


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_pose_timing.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-reps", type=int, default=5)
    ap.add_argument("--problems", type=int, default=512)
    a = ap.parse_args()
    import torch

    import homography_align_oracle as hao
    import homography_pose_scenes as S
    import matchinglib_poselib_amd as mpa
    from matchinglib_poselib_amd import _lib, pose

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"measured, one run, one MI355X: python tools/homography_pose_timing.py --reps {a.reps}" + (f" --parent-lib <parent build> --ab-reps {a.ab_reps}" if a.parent_lib else ""))
    say("wall time around calls that end in a synchronise; every shape warmed up; median [min .. max]; the restatement on one CPU thread of the same machine")
    ctx = mpa.Context(0)
    sm = torch.cuda.current_stream().cuda_stream
    for name in ("p3_n900", "p2_n4100"):
        sc = S.scene(name)
        n, P = len(sc["p1"]), sc["P"]
        d1, d2, dl = torch.from_numpy(sc["p1"]).cuda(), torch.from_numpy(sc["p2"]).cuda(), torch.from_numpy(sc["labels"]).cuda()
        R, t, E, info, norms, Hs = np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(24), np.zeros((P, 3)), np.zeros((P, 9))
        H0 = np.ascontiguousarray(sc["H0"], np.float64)

        def dev():
            rc = ctx.lib.mlpl_homography_alignment_dev(ctx.handle, d1.data_ptr(), d2.data_ptr(), dl.data_ptr(), n, P, sc["num_inl"].ctypes.data,
                                                       H0.ctypes.data, float(sc["th"]), R.ctypes.data, t.ctypes.data, E.ctypes.data, norms.ctypes.data,
                                                       Hs.ctypes.data, info.ctypes.data, sm)
            assert rc == 0 and info[0] == 0, _lib.last_error()

        td = timed(dev, a.reps)
        tc = timed(lambda: hao.alignment(sc["p1"], sc["p2"], sc["labels"], P, sc["H0"], sc["th"], 0), max(a.reps // 3, 5))
        rounds = int(info[2:10].sum())
        say(f"alignment alone, {name} (n = {n}, {P} planes, {rounds} rounds):")
        say(f"  mlpl_homography_alignment_dev:  {fmt(td)}")
        say(f"  restatement, one CPU thread:    {fmt(tc)}")
    sc = S.full_scene("full_three")
    d1, d2 = torch.from_numpy(sc["p1"]).cuda(), torch.from_numpy(sc["p2"]).cuda()
    res = {}

    def full_dev():
        st = np.array(FRESH, np.uint64)
        res["g"] = pose.pose_homographies_device(d1, d2, sc["th"], rng_state=st, ctx=ctx)
        torch.cuda.synchronize()

    def full_cpu():
        res["o"] = hao.pose_homographies(sc["p1"], sc["p2"], sc["th"], rng_state=np.array(FRESH, np.uint64))

    td, tc = timed(full_dev, a.reps), timed(full_cpu, max(a.reps // 3, 5))
    assert res["g"]["result"] == res["o"]["result"] == 0 and res["g"]["num_inl"].tolist() == res["o"]["num_inl"].tolist()
    say(f"whole function, full_three (n = {len(sc['p1'])}, planes {res['g']['num_inl'].tolist()}):")
    say(f"  mlpl_pose_homographies_dev:               {fmt(td)}")
    say(f"  the two restatements, one CPU thread:     {fmt(tc)}")
    # ---- a batch beside the loop of single calls ----
    B, cfg = a.problems, [c for c in S.FULL if c[0] == "full_three"][0]
    scenes = []
    seed = 0
    while len(scenes) < B:
        seed += 1
        try:
            scenes.append(S.pose_scene(cfg[1], cfg[2], seed, cfg[3], cfg[4]))
        except AssertionError:      # (a seed whose geometry puts a point behind a camera)
            pass
    th, stride = scenes[0]["th"], len(scenes[0]["p1"])
    h1, h2 = np.stack([s_["p1"] for s_ in scenes]), np.stack([s_["p2"] for s_ in scenes])
    b1, b2 = torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda()
    counts = np.full(B, stride, np.int32)
    mb, ml = torch.zeros((B, stride), dtype=torch.uint8, device="cuda"), torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
    res = {}

    def batch():
        st = np.tile(np.array(FRESH, np.uint64), (B, 1))
        res["batch"] = pose.pose_homographies_batch(b1, b2, counts, th, rng_states=st, masks_out=mb, ctx=ctx)
        torch.cuda.synchronize()

    def loop():
        out = []
        for b in range(B):
            st = np.array(FRESH, np.uint64)
            r = pose.pose_homographies_device(b1[b], b2[b], th, rng_state=st, ctx=ctx)
            ml[b] = r["mask"]
            r["rng_state"] = st
            out.append(r)
        torch.cuda.synchronize()
        res["loop"] = out

    batch(), loop()
    tb, tl = [], []
    for _ in range(5):
        for fn, ts in ((batch, tb), (loop, tl)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    same = bool((mb == ml).all().item()) and all(
        g["result"] == o["result"] and g["rng_state"].tobytes() == o["rng_state"].tobytes() and
        all(np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(o[k]).tobytes() for k in ("R", "t", "E", "H", "num_inl", "info"))
        for g, o in zip(res["batch"], res["loop"]))
    codes = {c: sum(1 for g in res["batch"] if g["result"] == c) for c in (0, -1, -2, -3)}
    hub = np.zeros(12, np.int64)
    ctx.lib.mlpl_arrsac_last_stats(ctx.handle, hub.ctypes.data)
    say(f"{B} problems like full_three (n = {stride}; result codes {codes}):")
    say(f"  one mlpl_pose_homographies_batch_dev call:    {fmt(tb)} = {np.median(tb) / B * 1e3:.1f} us per problem")
    say(f"  loop of {B} mlpl_pose_homographies_dev calls: {fmt(tl)} = {np.median(tl) / B * 1e3:.1f} us per problem")
    say(f"  batch equal to the loop by bytes (codes, R, t, E, planes, info, masks, stream states): {same}")
    ctx.close()
    if a.parent_lib:
        tool = os.path.join(ROOT, "tools", "homography_batch_timing.py")
        runs = {"parent": [], "this": []}
        for rep in range(a.ab_reps):
            pair = (("parent", a.parent_lib), ("this", _lib.library_path()))
            for who, path in (pair if rep % 2 == 0 else pair[::-1]):   # the build that goes first alternates too
                env = dict(os.environ, MLPL_LIB_PATH=path)
                out = subprocess.run([sys.executable, tool, "--child"], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
                runs[who].append(json.loads([ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1][6:]))
        same = all(r["H"] == runs["parent"][0]["H"] for rs in runs.values() for r in rs)
        say("existing entries, parent build and this build alternating, a fresh process per repetition (medians of 30 calls each):")
        for key, label in (("arrsac_dev", "mlpl_homography_arrsac_dev, n5000_half"), ("mult_dev", "mlpl_mult_homographies_dev, three")):
            for who in ("parent", "this"):
                say(f"  {label}, {who:6s} build:  {fmt([r[key] for r in runs[who]])}")
        say(f"  H of both entries identical in bytes across all runs and both builds: {same}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
