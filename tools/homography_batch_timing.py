"""The batched plane estimators beside a loop over the single entries, and the single entries of two BUILDS of the library.

  python tools/homography_batch_timing.py [--problems 512] [--reps 5] [--out profiles/homography_batch_timing.txt] [--parent-lib PATH]

One command measures everything (wall time around calls that end in a synchronise; every shape is warmed up first; the variants that are
compared alternate; every figure is repeated --reps times and printed as median [min .. max]):
  * 512 problems like scene n5000_half (seeds 1 ... 512, fresh streams per problem): one mlpl_homography_arrsac_batch_dev call against a loop
    of 512 mlpl_homography_arrsac_dev calls on one context;
  * 512 problems like scene three: mlpl_mult_homographies_batch_dev against the loop of mlpl_mult_homographies_labels_dev;
  * the sequential restatement (tests/cpp/homography_oracle.cpp) on ten scenes of either family, one CPU thread, scaled to 512;
  * with --parent-lib: mlpl_homography_arrsac_dev on n5000_half and mlpl_mult_homographies_dev on three (the two lines of
    profiles/homography_timing.txt) for the parent's build and this one, each in a fresh process per repetition, alternating.
The batch results are compared with the loop's by bytes as they are timed."""
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

import homography_scenes as hs

FRESH = (0xFFFFFFFF, 0xFFFFFFFF)


def fmt(ts):
    return f"median {np.median(ts):.3f} ms [min {min(ts):.3f} .. max {max(ts):.3f}] over {len(ts)}"


def child():
    """The two single entries on this process' build of the library (MLPL_LIB_PATH): medians of 30 calls each.  No torch, and the library
    is bound by hand: the package's loader insists on every symbol of THIS tree's header, which the parent's build does not export."""
    from matchinglib_poselib_amd import _lib

    class Ctx:
        pass

    ctx = Ctx()
    ctx.lib = C.CDLL(_lib.library_path())
    for name in ("mlpl_ctx_create", "mlpl_homography_arrsac_dev", "mlpl_mult_homographies_dev"):
        getattr(ctx.lib, name).restype, getattr(ctx.lib, name).argtypes = _lib._SIGNATURES[name]
    ctx.handle = C.c_void_p()
    assert ctx.lib.mlpl_ctx_create(0, C.byref(ctx.handle)) == 0
    ctx.lib.mlpl_ctx_destroy.argtypes = [C.c_void_p]
    ctx.close = lambda: ctx.lib.mlpl_ctx_destroy(ctx.handle)
    hip = C.CDLL("libamdhip64.so")            # the runtime the library itself is linked against
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes = [C.c_void_p, C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_dev(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p

    out = {}
    p1, p2, _, _, th = hs.single("n5000_half")
    d1, d2, dm = to_dev(p1), to_dev(p2), to_dev(np.zeros(5000, np.uint8))
    H, ninl = np.zeros(9), C.c_int(0)

    def one_plane():
        st = np.array(FRESH, np.uint64)
        rc = ctx.lib.mlpl_homography_arrsac_dev(ctx.handle, d1, d2, 5000, float(th), st.ctypes.data, H.ctypes.data, dm, C.byref(ninl), None, None)
        assert rc == 0 and hip.hipDeviceSynchronize() == 0

    q1, q2, _, _, th3 = hs.multi("three")
    e1, e2 = to_dev(q1), to_dev(q2)
    cap, npl = 31, C.c_int(0)
    Hs, num, stg, thu = np.zeros((cap, 9)), np.zeros(cap, np.int32), np.zeros(cap), np.zeros(cap)

    def three_planes():
        st = np.array(FRESH, np.uint64)
        rc = ctx.lib.mlpl_mult_homographies_dev(ctx.handle, e1, e2, 900, float(th3), 1, 0, 30, st.ctypes.data, cap, C.byref(npl), Hs.ctypes.data,
                                                num.ctypes.data, stg.ctypes.data, thu.ctypes.data, None, None)
        assert rc == 0 and npl.value == 3 and hip.hipDeviceSynchronize() == 0

    for name, fn in (("arrsac_dev", one_plane), ("mult_dev", three_planes)):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ts))
    out["H"] = H.view(np.uint64).tolist() + Hs[:3].view(np.uint64).ravel().tolist()
    ctx.close()
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_batch_timing.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    import torch

    import homography_oracle as ho
    import matchinglib_poselib_amd as mpa
    from matchinglib_poselib_amd import _lib

    B, reps = a.problems, max(a.reps, 5)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"measured, one run, one MI355X: python tools/homography_batch_timing.py --problems {B} --reps {reps}" + (" --parent-lib <parent build>" if a.parent_lib else ""))
    say("wall time around calls that end in a synchronise; every shape warmed up; batch and loop alternate; median [min .. max]")
    ctx = mpa.Context(0)
    lib, h = ctx.lib, ctx.handle
    sm = torch.cuda.current_stream().cuda_stream
    hub = np.zeros(12, np.int64)

    def pack(scenes, stride):
        p1, p2 = np.zeros((B, stride, 2)), np.zeros((B, stride, 2))
        for b, s in enumerate(scenes):
            p1[b], p2[b] = s[0], s[1]
        return torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()

    # ---- one plane ----
    n = 5000
    scenes = [hs.planes_scene(n, (2500,), seed, "pix", True) for seed in range(1, B + 1)]
    th = scenes[0][4]
    d1, d2 = pack(scenes, n)
    counts = np.full(B, n, np.int32)
    masks_b = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    masks_l = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    res = {}

    def plane_batch():
        st, H, ninl, status = np.tile(np.array(FRESH, np.uint64), (B, 1)), np.zeros((B, 9)), np.zeros(B, np.int32), np.zeros(B, np.int32)
        rc = lib.mlpl_homography_arrsac_batch_dev(h, B, d1.data_ptr(), d2.data_ptr(), n, counts.ctypes.data, float(th), st.ctypes.data, H.ctypes.data,
                                                  masks_b.data_ptr(), ninl.ctypes.data, status.ctypes.data, None, sm)
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        res["batch"] = (H, ninl, status, st)

    def plane_loop():
        st, H, ninl, status = np.tile(np.array(FRESH, np.uint64), (B, 1)), np.zeros((B, 9)), np.zeros(B, np.int32), np.zeros(B, np.int32)
        one = C.c_int(0)
        for b in range(B):
            status[b] = lib.mlpl_homography_arrsac_dev(h, d1[b].data_ptr(), d2[b].data_ptr(), n, float(th), st[b].ctypes.data, H[b].ctypes.data,
                                                       masks_l[b].data_ptr(), C.byref(one), None, sm)
            ninl[b] = one.value
        torch.cuda.synchronize()
        res["loop"] = (H, ninl, status, st)

    def alternate(f_batch, f_loop):
        f_batch(), f_loop()
        tb, tl = [], []
        for _ in range(reps):
            for f, ts in ((f_batch, tb), (f_loop, tl)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts.append((time.perf_counter() - t0) * 1e3)
        return tb, tl

    def verdict(tb, tl):
        spread = max(max(tb) - min(tb), max(tl) - min(tl))
        gain = np.median(tl) - np.median(tb)
        return (f"loop - batch = {gain:.3f} ms, largest spread {spread:.3f} ms: the batch call takes "
                + ("LESS wall time than the loop by more than the spread" if gain > spread else "NOT less wall time than the loop by more than the spread"))

    try:
        tb, tl = alternate(plane_batch, plane_loop)
        lib.mlpl_arrsac_last_stats(h, hub.ctypes.data)   # (the loop's single calls do not touch [8] / [9])
        same = all(res["batch"][k].tobytes() == res["loop"][k].tobytes() for k in range(4)) and torch.equal(masks_b, masks_l)
        say("")
        say(f"{B} problems like n5000_half (n = 5000, 2500 planted inliers, pixel units, seeds 1 ... {B}, fresh streams per problem); "
            f"{int((res['batch'][2] == 0).sum())} succeed, mean inliers {res['batch'][1].mean():.0f}; batch == loop by bytes: {same}")
        say(f"  one mlpl_homography_arrsac_batch_dev call:        {fmt(tb)} = {np.median(tb) / B * 1e3:.1f} us per problem")
        say(f"  loop of {B} mlpl_homography_arrsac_dev calls:     {fmt(tl)} = {np.median(tl) / B * 1e3:.1f} us per problem")
        say(f"  {verdict(tb, tl)}; ratio of the medians {np.median(tl) / np.median(tb):.1f}")
        say(f"  the hub in the batch call (last of the repetitions): rounds {hub[8]}, merged launches {hub[9]}")
    except Exception as e:   # a refused batch (an internal capacity, say) is a finding: it goes on the page
        say(f"  the one-plane section ended early: {e}")
    del d1, d2, masks_b, masks_l

    # ---- three planes ----
    n3, cap = 900, 31
    scenes3 = [hs.planes_scene(n3, (380, 220, 120), seed, "cam", True) for seed in range(1, B + 1)]
    th3 = scenes3[0][4]
    e1, e2 = pack(scenes3, n3)
    counts3 = np.full(B, n3, np.int32)
    lab_b = torch.full((B, n3), -1, dtype=torch.int32, device="cuda")
    lab_l = torch.full((B, n3), -1, dtype=torch.int32, device="cuda")

    def outs():
        return [np.tile(np.array(FRESH, np.uint64), (B, 1)), np.zeros(B, np.int32), np.zeros((B, cap, 9)), np.zeros((B, cap), np.int32), np.zeros((B, cap)),
                np.zeros((B, cap)), np.zeros((B, cap), np.int32)]

    def mult_batch():
        o, status = outs(), np.zeros(B, np.int32)
        rc = lib.mlpl_mult_homographies_batch_dev(h, B, e1.data_ptr(), e2.data_ptr(), n3, counts3.ctypes.data, float(th3), 1, 0, 30, o[0].ctypes.data, cap,
                                                  o[1].ctypes.data, o[2].ctypes.data, o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data, o[6].ctypes.data,
                                                  lab_b.data_ptr(), status.ctypes.data, sm)
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        res["mbatch"] = o

    def mult_loop():
        o = outs()
        one = C.c_int(0)
        for b in range(B):
            rc = lib.mlpl_mult_homographies_labels_dev(h, e1[b].data_ptr(), e2[b].data_ptr(), n3, float(th3), 1, 0, 30, o[0][b].ctypes.data, cap, C.byref(one),
                                                       o[2][b].ctypes.data, o[3][b].ctypes.data, o[4][b].ctypes.data, o[5][b].ctypes.data, o[6][b].ctypes.data,
                                                       lab_l[b].data_ptr(), None, sm)
            assert rc == 0, _lib.last_error()
            o[1][b] = one.value
        torch.cuda.synchronize()
        res["mloop"] = o

    try:
        tb, tl = alternate(mult_batch, mult_loop)
        lib.mlpl_arrsac_last_stats(h, hub.ctypes.data)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(res["mbatch"], res["mloop"])) and torch.equal(lab_b, lab_l)
        say("")
        say(f"{B} problems like three (n = 900, planes of 380 / 220 / 120, camera units, minPtsPerPlane = 30, seeds 1 ... {B}); planes found: "
            f"{np.bincount(np.maximum(res['mbatch'][1], 0)).tolist()} problems with 0, 1, 2 ... planes; batch == loop by bytes: {same}")
        say(f"  one mlpl_mult_homographies_batch_dev call:            {fmt(tb)} = {np.median(tb) / B * 1e3:.1f} us per problem")
        say(f"  loop of {B} mlpl_mult_homographies_labels_dev calls:  {fmt(tl)} = {np.median(tl) / B * 1e3:.1f} us per problem")
        say(f"  {verdict(tb, tl)}; ratio of the medians {np.median(tl) / np.median(tb):.1f}")
        say(f"  the hub in the batch call (last of the repetitions): rounds {hub[8]}, merged launches {hub[9]}")
    except Exception as e:
        say(f"  the three-plane section ended early: {e}")

    # ---- the sequential restatement, one CPU thread ----
    say("")
    say("sequential restatement (tests/cpp/homography_oracle.cpp), one CPU thread of the same machine, ten scenes of either family:")
    for name, fn in (("n5000_half-like", lambda s: ho.homography_arrsac(s[0], s[1], s[4])),
                     ("three-like", lambda s: ho.mult_homographies(s[0], s[1], s[4], min_pts_per_plane=30, cap=cap))):
        src = scenes if name.startswith("n5000") else scenes3
        fn(src[0])
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for s in src[:10]:
                fn(s)
            ts.append((time.perf_counter() - t0) * 1e3)
        say(f"  {name}: ten scenes {fmt(ts)}; SCALED to {B} problems (x {B / 10:.1f}, not measured at that count): {np.median(ts) * B / 10:.0f} ms")
    ctx.close()

    # ---- the single entries of two builds ----
    say("")
    if not a.parent_lib:
        say("single entries, parent's build against this one: not measured (no --parent-lib)")
    else:
        this_lib = _lib.library_path()
        got = {"parent": [], "this": []}
        for _ in range(reps):
            for which, path in (("parent", a.parent_lib), ("this", this_lib)):
                env = dict(os.environ, MLPL_LIB_PATH=os.path.abspath(path))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
                row = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
                if r.returncode != 0 or not row:
                    say(f"  the {which} build's process failed ({r.returncode}): {r.stderr[-300:]}")
                    return finish(a, lines)
                got[which].append(json.loads(row[0][6:]))
        say("single entries (the two lines of profiles/homography_timing.txt), a fresh process per repetition, parent's build and this one alternating; "
            "each figure the median of 30 calls:")
        for key, what in (("arrsac_dev", "mlpl_homography_arrsac_dev, n5000_half"), ("mult_dev", "mlpl_mult_homographies_dev, three")):
            p, t = [g[key] for g in got["parent"]], [g[key] for g in got["this"]]
            spread = max(p) - min(p)
            diff = np.median(t) - np.median(p)
            say(f"  {what}: parent {fmt(p)}; this build {fmt(t)}")
            say(f"    this - parent = {diff:+.4f} ms, spread of the parent alone {spread:.4f} ms: " + ("within the spread" if abs(diff) <= spread else
                                                                                                   ("FASTER than the spread explains" if diff < 0 else "SLOWER than the spread explains")))
        say(f"  results of the two builds equal by bytes: {all(g['H'] == got['parent'][0]['H'] for g in got['parent'] + got['this'])}")
    finish(a, lines)


def finish(a, lines):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
