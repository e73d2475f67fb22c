"""Generates the golden vectors under tests/golden/ (run in the build container, where /root/reference exists):

    make -C oracle ref && python tests/golden/make_golden.py

Matching vectors: inputs from matchinglib_poselib_amd.synth, expected (idx, dist) from two independent sources:
the reference's vendored NMSLIB seq_search (oracle/_ref/nmslib_knn, built from /root/reference sources in place)
for the distances and the tie-free indices, and a numpy brute force with lexicographic (dist, idx) selection for
the cvflann tie order.  Fixtures are data only (inputs + expected outputs).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib  # noqa: E402
from matchinglib_poselib_amd import synth  # noqa: E402


def run_nmslib(mode, q, t):
    tool = oracle_lib.ref_tool("nmslib_knn")
    assert tool, "build oracle/_ref first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            np.array([q.shape[0], t.shape[0], q.shape[1]], np.int32).tofile(f)
            q.tofile(f)
            t.tofile(f)
        subprocess.run([tool, mode, fin, fout], check=True)
        n = q.shape[0] * 2
        if mode.startswith("hamming"):
            raw = np.fromfile(fout, np.int32)
            return raw[:n].reshape(-1, 2), raw[n:].reshape(-1, 2)
        idx = np.fromfile(fout, np.int32, count=n).reshape(-1, 2)
        dist = np.fromfile(fout, np.float32, offset=4 * n).reshape(-1, 2)
        return idx, dist


def hamming_case(name, q, t):
    idx, dist = oracle_lib.numpy_knn_hamming(q, t)
    nidx, ndist = run_nmslib("hamming", q, t)
    assert np.array_equal(dist, ndist), "NMSLIB distances disagree with numpy brute force"
    lut = np.array([bin(i).count("1") for i in range(256)], np.int32)
    tie_free = np.zeros(q.shape[0], bool)
    for i in range(q.shape[0]):
        d = lut[np.bitwise_xor(t, q[i][None, :])].sum(axis=1)
        tie_free[i] = (d <= dist[i, 1]).sum() == 2 and dist[i, 0] < dist[i, 1]
    assert np.array_equal(idx[tie_free], nidx[tie_free])
    keep = dist[:, 0].astype(np.float32) < np.float32(0.75) * dist[:, 1].astype(np.float32)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), q=q, t=t, idx=idx, dist=dist, nms_idx=nidx,
                        nms_tie_free=tie_free, match_q=np.nonzero(keep)[0].astype(np.int32),
                        match_t=idx[keep, 0])
    print(name, q.shape, t.shape, "tie-free", int(tie_free.sum()), "matches", int(keep.sum()))


def main():
    q, t = synth.orb_pair(257, 263, seed=20260111)
    hamming_case("hamming_257x263", q, t)
    # adversarial ties: duplicated train rows, zero descriptors, exact copies as queries
    rng = np.random.default_rng(20260112)
    t = rng.integers(0, 256, (80, 32), dtype=np.uint8)
    t[7] = t[5]; t[33] = t[5]; t[60] = 0; t[61] = 0; t[79] = t[0]
    q = rng.integers(0, 256, (96, 32), dtype=np.uint8)
    q[:20] = t[:20]
    q[20] = 0
    q[21:40] = t[40:59] ^ np.uint8(1)
    hamming_case("hamming_ties_96x80", q, t)
    q, t = synth.orb_pair(2048, 2048, seed=20260101)  # BASELINE config C1
    hamming_case("hamming_c1_2048", q, t)




# ---- 5-point solver vectors: inputs + E-sets of the reference's vendored OpenGV fivept_nister ----------------
def run_opengv(pts):
    tool = oracle_lib.ref_tool("opengv_5pt")
    assert tool, "build oracle/_ref first: make -C oracle ref"
    ns, npts = pts.shape[:2]
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            np.array([ns, npts], np.int32).tofile(f)
            np.ascontiguousarray(pts, np.float64).tofile(f)
        subprocess.run([tool, fin, fout], check=True)
        raw = np.fromfile(fout, np.uint8).reshape(ns, 4 + 720)
    cnt = raw[:, :4].copy().view(np.int32)[:, 0]
    Es = raw[:, 4:].copy().view(np.float64).reshape(ns, 10, 3, 3)
    return cnt, Es


def fivept_case():
    p1, p2, R, t, mask, th = synth.pose_scene(5000, seed=20260103)
    rng = np.random.default_rng(20260113)
    ns = 120
    samples = np.stack([rng.choice(5000, 5, replace=False) for _ in range(ns)]).astype(np.int32)
    pts = np.concatenate([p1[samples], p2[samples]], axis=2)  # ns x 5 x (x1,y1,x2,y2)
    cnt, Es = run_opengv(pts)
    np.savez_compressed(os.path.join(HERE, "fivept_opengv_120.npz"), pts=pts, count=cnt, E=Es)
    print("fivept_opengv_120: mean #solutions", cnt.mean())


def nms_wrapper_case():
    """BRUTEFORCENMS: expected (idx, dist) straight from the reference's vendored NMSLIB driven with the reference
    wrapper's own packing (2 bytes per int, no length word => last 2 bytes ignored) and its 'l2' space (sqrt distances)."""
    out = {}
    for nb in (32, 31):
        q, t = synth.orb_pair(200, 260, nbytes=nb, seed=20260120 + nb)
        idx, dist = run_nmslib("hamming_wrapper", q, t)
        out[f"u8_{nb}_q"], out[f"u8_{nb}_t"], out[f"u8_{nb}_idx"], out[f"u8_{nb}_dist"] = q, t, idx, dist
    rng = np.random.default_rng(20260121)
    t = rng.normal(size=(260, 64)).astype(np.float32)
    q = rng.normal(size=(200, 64)).astype(np.float32)
    q[:60] = t[:60] + rng.normal(size=(60, 64)).astype(np.float32) * 0.05
    idx, dist = run_nmslib("l2", q, t)
    out["f32_q"], out["f32_t"], out["f32_idx"], out["f32_dist"] = q, t, idx, dist
    np.savez_compressed(os.path.join(HERE, "bruteforce_nms.npz"), **out)
    print("bruteforce_nms: ok")


# ---- G2: squared-L2 2-NN on integer-valued SIFT-like descriptors ---------------------------------------------------
def l2_case():
    """Exact d^2 (integers < 2^24) by numpy int64 brute force with lexicographic (d^2, idx) selection = the cvflann order;
    cross-checked against the reference's vendored NMSLIB `l2` space (sqrt distances, tie-free indices)."""
    out = {}
    for tag, (nq, nt, dim) in {"sift128": (300, 411, 128), "d64": (130, 257, 64)}.items():
        q, t = synth.sift_pair(nq, nt, dim=dim, seed=20260130 + dim)
        if tag == "d64":  # adversarial ties: duplicated train rows and exact copies as queries
            t[17] = t[3]; t[200] = t[3]; q[:10] = t[:10]
        qi, ti = q.astype(np.int64), t.astype(np.int64)
        idx = np.empty((nq, 2), np.int32)
        d2 = np.empty((nq, 2), np.int64)
        tie_free = np.zeros(nq, bool)
        for i in range(nq):
            d = ((ti - qi[i][None, :]) ** 2).sum(axis=1)
            order = np.lexsort((np.arange(nt), d))[:2]
            idx[i], d2[i] = order, d[order]
            tie_free[i] = (d <= d[order[1]]).sum() == 2 and d[order[0]] < d[order[1]]
        assert d2.max() < (1 << 24)
        nidx, ndist = run_nmslib("l2", q, t)
        assert np.array_equal(ndist, np.sqrt(d2.astype(np.float32))), "NMSLIB l2 distances disagree with the exact integers"
        assert np.array_equal(nidx[tie_free], idx[tie_free])
        keep = d2[:, 0].astype(np.float32) < np.float32(0.75) * d2[:, 1].astype(np.float32)
        out.update({f"{tag}_q": q, f"{tag}_t": t, f"{tag}_idx": idx, f"{tag}_d2": d2.astype(np.float32), f"{tag}_nms_idx": nidx,
                    f"{tag}_tie_free": tie_free, f"{tag}_match_q": np.nonzero(keep)[0].astype(np.int32)})
        print("l2", tag, q.shape, t.shape, "tie-free", int(tie_free.sum()), "matches", int(keep.sum()))
    np.savez_compressed(os.path.join(HERE, "l2_integer_sift.npz"), **out)


# ---- G4: glibc srand/rand stream (from libc itself) + compact runRANSAC trace of the CPU restatement --------------------
def ransac_case():
    import ctypes
    import zlib
    libc = ctypes.CDLL("libc.so.6")
    seeds = np.array([0, 1, 12345, 20260103, 4294967295], np.uint32)
    head = np.empty((len(seeds), 2000), np.int32)
    crc = np.empty(len(seeds), np.uint32)
    for k, sd in enumerate(seeds):
        libc.srand(ctypes.c_uint(int(sd)))
        stream = np.array([libc.rand() for _ in range(100000)], np.int32)
        head[k] = stream[:2000]
        crc[k] = zlib.crc32(stream.tobytes())
    ora = oracle_lib.load()
    out = dict(rand_seeds=seeds, rand_head=head, rand_crc32_100000=crc)
    # scene = C3's generator at the reference's own settings (1000 iterations, confidence 0.999) and a no-early-exit run
    for tag, (n, conf, iters, seed) in {"ref": (5000, 0.999, 1000, 12345), "full": (800, 1.0, 400, 7)}.items():
        p1, p2, R, t, mask, th = synth.pose_scene(n, seed=20260103)
        o = ora.ransac_essential(p1, p2, th, confidence=conf, max_iters=iters, lesqu=False, seed=seed, trace=True)
        k = o["iters"]
        tr = o["trace"]
        out.update({
            f"{tag}_params": np.array([n, conf, iters, seed, th], np.float64),
            f"{tag}_iters": np.int32(k), f"{tag}_n_inliers": np.int32(o["n_inliers"]), f"{tag}_E": o["E"], f"{tag}_mask": np.packbits(o["mask"]),
            f"{tag}_idx": np.array([list(tr[i].idx) for i in range(k)], np.int32),
            f"{tag}_nmodels": np.array([tr[i].nmodels for i in range(k)], np.int8),
            f"{tag}_good": np.array([list(tr[i].good) for i in range(k)], np.int16),
            f"{tag}_err_sum": np.array([list(tr[i].err_sum) for i in range(k)], np.float64),
            f"{tag}_niters_after": np.array([tr[i].niters_after for i in range(k)], np.int32),
            f"{tag}_best_taken": np.array([tr[i].best_taken for i in range(k)], np.int8)})
        lo = ora.ransac_essential(p1, p2, th, confidence=conf, max_iters=iters, lesqu=True, seed=seed)
        out.update({f"{tag}_refit_E": lo["E"], f"{tag}_refit_mask": np.packbits(lo["mask"]), f"{tag}_refit_n_inliers": np.int32(lo["n_inliers"])})
        print("ransac", tag, "iters", k, "inliers", o["n_inliers"], "refit inliers", lo["n_inliers"])
    np.savez_compressed(os.path.join(HERE, "ransac_trace.npz"), **out)


# ---- G5: cheirality / pose recovery on scenes with a known (R, t) -----------------------------------------------------
def cheirality_case():
    """Noise-free correspondences of a known pose, with far points (z >= dist), points behind one camera (mirrored input) and an
    input mask; expected = analytic truth (R, t, which points pass z > 0 in both views and z < dist) AND the CPU restatement's
    outputs (count, mask, R, t, Q)."""
    ora = oracle_lib.load()
    rng = np.random.default_rng(20260140)
    out = {}
    for tag, (axis, deg, tt) in {"a": ((0.2, 0.9, 0.1), 5.0, (1.0, 0.05, -0.02)), "b": ((-0.5, 0.3, 0.8), 12.0, (-0.2, 0.1, 1.0))}.items():
        R = synth._rot(axis, deg)
        t = np.asarray(tt, float)
        t /= np.linalg.norm(t)
        n = 400
        X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], axis=1)
        X[:40, 2] = rng.uniform(60, 200, 40)                 # far points: fail z < dist (dist = 50)
        X[40:60, 2] = rng.uniform(49.0, 51.0, 20)            # around the distance gate
        p1 = X[:, :2] / X[:, 2:3]
        X2 = X @ R.T + t
        p2 = X2[:, :2] / X2[:, 2:3]
        p1[60:80] = -p1[60:80]                               # inconsistent pairs: land behind a camera for the true pose
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E = tx @ R
        m_in = (rng.random(n) < 0.85).astype(np.uint8)
        for variant, (Ein, mk) in {"plain": (E, None), "neg_scaled_masked": (-3.7 * E, m_in)}.items():
            good, Ro, to, Qo, mo = ora.recover_pose(Ein, p1, p2, 50.0, mk)
            truth_ok = (X[:, 2] < 50.0)
            truth_ok[60:80] = False
            key = f"{tag}_{variant}"
            out.update({f"{key}_E": Ein, f"{key}_good": np.int32(good), f"{key}_R": Ro, f"{key}_t": to, f"{key}_Q": Qo,
                        f"{key}_mask_out": (mo if mo is not None else np.zeros(0, np.uint8))})
            assert np.abs(Ro - R).max() < 1e-9 and np.abs(to - t).max() < 1e-9, "restatement does not recover the known pose"
        out.update({f"{tag}_p1": p1, f"{tag}_p2": p2, f"{tag}_R_true": R, f"{tag}_t_true": t, f"{tag}_X_true": X, f"{tag}_mask_in": m_in,
                    f"{tag}_truth_ok": truth_ok})
        print("cheirality", tag, "good", good)
    np.savez_compressed(os.path.join(HERE, "cheirality.npz"), **out)


# ---- reference's own coefficient arithmetic (getCoeffMat + c[0..10]) compiled in place: oracle/_ref/libfivept_ref.so ----
def coeff_case():
    import ctypes as C
    so = os.path.join(ROOT, "oracle", "_ref", "libfivept_ref.so")
    assert os.path.exists(so), "build oracle/_ref first: make -C oracle ref"
    ref = C.CDLL(so)
    rng = np.random.default_rng(20260150)
    n = 40
    EE = np.empty((n, 4, 9))
    A = np.empty((n, 10, 20))
    b = rng.normal(size=(n, 3, 13))
    c = np.empty((n, 11))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(9, 9)))
        EE[i] = Q[:, :4].T
        e = np.ascontiguousarray(EE[i]).copy()
        a = np.zeros(200)
        ref.ref_getCoeffMat(C.c_void_p(e.ctypes.data), C.c_void_p(a.ctypes.data))
        A[i] = a.reshape(10, 20)
        bi = np.ascontiguousarray(b[i])
        ci = np.zeros(11)
        ref.ref_detpoly(C.c_void_p(bi.ctypes.data), C.c_void_p(ci.ctypes.data))
        c[i] = ci
    np.savez_compressed(os.path.join(HERE, "coeff_ref.npz"), EE=EE, A=A, b=b, c=c)
    print("coeff_ref: ok")


def eigen_svd_case():
    """Eigen::JacobiSVD<Matrix3d> of the Eigen 3.2.0 the reference vendors (oracle/_ref/eigen_svd3): singular values, U, V with
    Eigen's column signs, for random matrices, near-essential matrices (the ValidModel regime) and their negatives."""
    import struct
    import tempfile
    tool = os.path.join(ROOT, "oracle", "_ref", "eigen_svd3")
    rng = np.random.default_rng(20260301)
    Ms = rng.standard_normal((600, 3, 3))
    for i in range(300):
        u, _, vt = np.linalg.svd(Ms[i])
        Ms[i] = u @ np.diag([1.0, 1.0 + 0.15 * rng.random(), 0.02 * rng.random()]) @ vt
    Ms = np.concatenate([Ms, -Ms[:100]])
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "i.bin"), os.path.join(d, "o.bin")
        open(fi, "wb").write(struct.pack("i", len(Ms)) + Ms.tobytes())
        subprocess.run([tool, fi, fo], check=True)
        out = np.fromfile(fo).reshape(-1, 21)
    np.savez_compressed(os.path.join(HERE, "eigen_svd3.npz"), M=Ms, sv=out[:, :3], U=out[:, 3:12].reshape(-1, 3, 3),
                        V=out[:, 12:].reshape(-1, 3, 3))
    print("eigen_svd3: ok", len(Ms))


def arrsac_case():
    """ARRSAC fixture (oracle-generated, like the RANSAC trace): scenes, the cv::RNG stream head, and per scene the oracle's
    result + statistics + the first 60 turns of its first stage."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    from matchinglib_poselib_amd import synth
    ora = oracle_lib.load()
    out = {}
    stream, st = ora.cv_rng_stream(0xFFFFFFFF, 64)
    out["rng_head"], out["rng_state_after"] = stream, np.array([st], np.uint64)
    ora.lib.oracle_arrsac_trace.argtypes = [C.c_void_p, C.c_int]
    cases = [(1500, 0.5, 20260401), (400, 0.7, 20260402), (90, 0.6, 20260403), (1200, 0.92, 20260404)]
    out["cases"] = np.array(cases, np.float64)
    for ci, (n, frac, seed) in enumerate(cases):
        p1, p2, R, t, truth, th = synth.pose_scene(n, frac, seed=seed)
        buf = np.zeros(20 * 4000, np.int32)
        ora.lib.oracle_arrsac_trace(buf.ctypes.data, len(buf))
        o = ora.arrsac_essential(p1, p2, th, refine=True)
        ln = ora.lib.oracle_arrsac_trace(None, 0)
        out[f"c{ci}_p1"], out[f"c{ci}_p2"], out[f"c{ci}_th"] = p1, p2, np.array([th])
        out[f"c{ci}_ok"], out[f"c{ci}_E"], out[f"c{ci}_mask"] = np.array([o["ok"]]), o["E"], np.packbits(o["mask"])
        out[f"c{ci}_stats"], out[f"c{ci}_rng"] = o["stats"], o["rng_state"]
        out[f"c{ci}_turns"] = buf[:ln].reshape(-1, 20)[:60].copy()
    np.savez_compressed(os.path.join(HERE, "arrsac_trace.npz"), **out)
    print("arrsac_trace: ok")


USAC_CASES = [(5000, 0.5, 20260103), (300, 0.5, 13), (1200, 0.9, 15), (150, 0.6, 16), (64, 0.8, 18), (4000, 0.4, 19), (2000, 0.7, 12),
              (600, 0.35, 21)]


USAC_EVENTS_KEPT = 700


def usac_scene(n, frac, seed):
    """Scene + PROSAC order (a noisy quality score: inliers tend to come first) of one USAC fixture case."""
    from matchinglib_poselib_amd import synth
    p1, p2, R, t, truth, th = synth.pose_scene(n, frac, seed=seed)
    score = np.random.default_rng(seed).random(n) + 0.6 * (~truth)
    return p1, p2, th, truth, np.argsort(score, kind="stable").astype(np.uint32)


def usac_case():
    """USAC fixture: decision traces of the REFERENCE's USAC.h (include/usac/estimators/USAC.h) + usac/utils compiled in place
    (oracle/_ref/usac_ref).  Two solver modes per case: `--solver-oracle` (the minimal models come from the oracle's 5-point solver, so
    the trace pins the control-flow restatement decision by decision) and OpenGV (the reference's own solver: final results only, its
    unconverged roots make the traces part).  Cases where ccmath's svdu1v / svduv (the reference's 9 x 9 / 3 x 3 decompositions) stop
    early are recorded with agree = 0: there the reference's refined model is inaccurate and the oracle's Jacobi iteration is not."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle_lib
    import usac_compare
    import usac_ref_tool as u
    ora = oracle_lib.load()
    out = {"cases": np.array(USAC_CASES, np.float64)}
    k = 0
    for (n, frac, seed) in USAC_CASES:
        p1, p2, th, truth, order = usac_scene(n, frac, seed)
        for prosac in (0, 1):
            for usac_seed in (12345, 7):
                si = order if prosac else None
                r = u.run(p1, p2, th, usac_seed, sorted_idx=si, solver_oracle=True)
                g = u.run(p1, p2, th, usac_seed, sorted_idx=si)
                o = ora.usac_essential(p1, p2, th, usac_seed, sorted_idx=si, event_cap=200000)
                first, d = usac_compare.compare(r["events"], o["events"])
                agree = int(first is None and np.array_equal(r["flags"], o["flags"]))
                out[f"k{k}_meta"] = np.array([n, frac, seed, prosac, usac_seed, agree], np.float64)
                out[f"k{k}_events"] = r["events"][:USAC_EVENTS_KEPT]   # the head of the trace + its length; the final record pins the rest
                out[f"k{k}_n_events"] = np.array([len(r["events"])])
                out[f"k{k}_final"], out[f"k{k}_E"], out[f"k{k}_flags"] = r["final"], r["E"], np.packbits(r["flags"])
                out[f"k{k}_pool_head"] = r["pool"][:64]
                out[f"k{k}_opengv_final"], out[f"k{k}_opengv_flags"] = g["final"], np.packbits(g["flags"])
                print(f"usac case {k}: n {n} prosac {prosac} seed {usac_seed}: events {len(r['events'])} agree {agree} "
                      f"inliers ref/opengv {int(r['final'][5])}/{int(g['final'][5])} hyps {int(r['final'][1])}/{int(g['final'][1])}")
                k += 1
    out["n_cases"] = np.array([k])
    np.savez_compressed(os.path.join(HERE, "usac_trace.npz"), **out)
    print("usac_trace: ok", os.path.getsize(os.path.join(HERE, "usac_trace.npz")), "bytes")


USAC_STEWENIUS_CASES = [(5000, 0.5, 20260103), (300, 0.5, 13), (1200, 0.9, 15), (8192, 0.25, 14), (800, 0.3, 11), (2000, 0.7, 12)]
USAC_STEWENIUS_EVENTS_KEPT = 400


def usac_stewenius_case():
    """USAC with the reference's DEFAULT minimal solver: ConfigUSAC (pose_estim.h:99) and the harness (main.cpp:608, cfgUSAC 311220) select
    POSE_STEWENIUS, i.e. OpenGV's fivept_stewenius filtered for real solutions (EssentialMatEstimator.h:456-489), with mS = 6 and
    tM = 2736 on a process' first call (usac_estimations.cpp:323, 412, 422).  `usac_ref --stewenius` runs exactly that on the
    reference-built USAC.h + OpenGV; only the order convention of a sample's solutions is put on top (Eigen::EigenSolver's order of ten
    eigenvalues is not restated).  Unlike fivept_nister's bracketing the eigenvalue solver is converged to rounding, so these traces hold
    the oracle's and the device's OWN five-point solver -- not a swapped-in one -- to the reference's, decision by decision.
    agree = 0 marks runs that part at a refit where ccmath's svdu1v stops early (usac_case)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle_lib
    import usac_compare
    import usac_ref_tool as u
    ora = oracle_lib.load()
    out = {"cases": np.array(USAC_STEWENIUS_CASES, np.float64)}
    k = 0
    for (n, frac, seed) in USAC_STEWENIUS_CASES:
        p1, p2, th, truth, order = usac_scene(n, frac, seed)
        for prosac in (0, 1):
            for usac_seed in (12345, 7):
                si = order if prosac else None
                r = u.run(p1, p2, th, usac_seed, sorted_idx=si, stewenius=True, sprt_ms=6.0, sprt_tm=2736.0)
                o = ora.usac_essential(p1, p2, th, usac_seed, sorted_idx=si, event_cap=200000, sprt_ms=6.0, sprt_tm=2736.0)
                first, d = usac_compare.compare(r["events"], o["events"])
                agree = int(first is None and np.array_equal(r["flags"], o["flags"]))
                out[f"k{k}_meta"] = np.array([n, frac, seed, prosac, usac_seed, agree], np.float64)
                out[f"k{k}_events"] = r["events"][:USAC_STEWENIUS_EVENTS_KEPT]
                out[f"k{k}_n_events"] = np.array([len(r["events"])])
                out[f"k{k}_final"], out[f"k{k}_E"], out[f"k{k}_flags"] = r["final"], r["E"], np.packbits(r["flags"])
                print(f"usac stewenius case {k}: n {n} prosac {prosac} seed {usac_seed}: events {len(r['events'])} agree {agree} first {first} "
                      f"inliers {int(r['final'][5])} hyps {int(r['final'][1])} {d}")
                k += 1
    out["n_cases"] = np.array([k])
    np.savez_compressed(os.path.join(HERE, "usac_stewenius_trace.npz"), **out)
    print("usac_stewenius_trace: ok", os.path.getsize(os.path.join(HERE, "usac_stewenius_trace.npz")), "bytes")


USAC_REFINE_CASES = [(5000, 0.5, 20260103), (300, 0.5, 13), (1200, 0.9, 15), (800, 0.3, 11), (2000, 0.7, 12), (150, 0.6, 16)]
USAC_REFINE_EVENTS_KEPT = 300


def usac_refine_case():
    """USAC with the inner refinements of the 5-point family (poselib::RefineAlg 4..7; EssentialMatEstimator.h:640-850, findWeights
    :2404-2428) -- ConfigUSAC's default is REF_STEWENIUS_WEIGHTS (5) with POSE_STEWENIUS (pose_estim.h:99-100).
    refine 5 / 4 (Stewenius with / without the pseudo-Huber weights): `usac_ref --stewenius`, i.e. the reference-built USAC.h with
    OpenGV's fivept_stewenius as the minimal AND the refinement solver (weighted rows through the reference-built
    modules::fivept_stewenius_main), mS = 6, tM = 2736: nothing swapped in, only the order convention on top.  The oracle's own solver
    follows these traces event by event in 48 of 48 runs.
    refine 7 / 6 (Nister): OpenGV's fivept_nister returns unconverged roots on a share of its inputs (usac_case), so the event traces come
    from `--solver-oracle` (control flow pinned, solver swapped) and the reference solver's own run contributes its final counts."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle_lib
    import usac_compare
    import usac_ref_tool as u
    ora = oracle_lib.load()
    out = {"cases": np.array(USAC_REFINE_CASES, np.float64)}
    k = 0
    kw = dict(sprt_ms=6.0, sprt_tm=2736.0)
    for refine in (5, 4, 7, 6):
        for (n, frac, seed) in USAC_REFINE_CASES:
            p1, p2, th, truth, order = usac_scene(n, frac, seed)
            for prosac in (0, 1):
                for usac_seed in (12345, 7):
                    if refine in (4, 6) and usac_seed == 7:
                        continue                      # the unweighted forms: half the runs
                    si = order if prosac else None
                    if refine in (4, 5):
                        r = u.run(p1, p2, th, usac_seed, refine=refine, sorted_idx=si, stewenius=True, **kw)
                    else:
                        r = u.run(p1, p2, th, usac_seed, refine=refine, sorted_idx=si, solver_oracle=True, **kw)
                        gres = u.run(p1, p2, th, usac_seed, refine=refine, sorted_idx=si, **kw)
                        out[f"k{k}_opengv_final"], out[f"k{k}_opengv_flags"] = gres["final"], np.packbits(gres["flags"])
                    o = ora.usac_essential(p1, p2, th, usac_seed, refine=refine, sorted_idx=si, event_cap=400000, **kw)
                    first, d = usac_compare.compare(r["events"], o["events"])
                    agree = int(first is None and np.array_equal(r["flags"], o["flags"]))
                    out[f"k{k}_meta"] = np.array([n, frac, seed, prosac, usac_seed, agree, refine], np.float64)
                    out[f"k{k}_events"] = r["events"][:USAC_REFINE_EVENTS_KEPT]
                    out[f"k{k}_n_events"] = np.array([len(r["events"])])
                    out[f"k{k}_final"], out[f"k{k}_E"], out[f"k{k}_flags"] = r["final"], r["E"], np.packbits(r["flags"])
                    print(f"usac refine case {k}: refine {refine} n {n} prosac {prosac} seed {usac_seed}: events {len(r['events'])} agree {agree} "
                          f"first {first} inliers {int(r['final'][5])} hyps {int(r['final'][1])} {d}")
                    k += 1
    out["n_cases"] = np.array([k])
    np.savez_compressed(os.path.join(HERE, "usac_refine_trace.npz"), **out)
    print("usac_refine_trace: ok", os.path.getsize(os.path.join(HERE, "usac_refine_trace.npz")), "bytes")


def degen_math_case():
    """Fixture for the host numerics of USAC's degeneracy handling: the reference's vendored OpenGV (twopt_rotationOnly, rotationOnly,
    twopt, eigensolver) and PoseTools error functions compiled in place (oracle/_ref/opengv_degen) on three scenes -- pure rotation,
    short baseline, general motion.  The eigensolver rows are kept for what they are: its Levenberg-Marquardt differentiates the
    gradient by forward differences with a step of 1.5e-8 |x|, so its path follows the rounding noise of the build; the tests use them
    with that in mind (tests/test_usac_degen_math.py)."""
    import struct
    import subprocess
    import tempfile
    from matchinglib_poselib_amd import synth

    tool = os.path.join(ROOT, "oracle", "_ref", "opengv_degen")
    out = {}
    K, m = 48, 24
    for s, (name, kw) in enumerate((("rotation", dict(t_len=0.0)), ("shortbase", dict(t_len=0.05)), ("general", {}))):
        n = 300
        p1, p2, R, t, truth, th = synth.pose_scene(n, 0.8, seed=50 + s, **kw)
        rng = np.random.default_rng(70 + s)
        inl = np.flatnonzero(truth)
        pairs = np.stack([rng.choice(inl, 2, replace=False) for _ in range(K)]).astype(np.int32)
        lists = np.stack([rng.choice(inl, m, replace=False) for _ in range(K)]).astype(np.int32)
        fives = np.stack([rng.choice(inl, 5, replace=False) for _ in range(K)]).astype(np.int32)
        # start rotations: identity for the first half, the true inverse rotation (view 2 -> view 1 of the adapter) perturbed for the rest
        Rs = np.tile(np.eye(3).reshape(1, 9), (K, 1))
        for k in range(K // 2, K):
            w = rng.normal(0, 0.01, 3)
            Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            Rs[k] = ((np.eye(3) + Wx) @ R).reshape(9)
        pts = np.concatenate([p1, p2], 1).astype(np.float64)
        with tempfile.TemporaryDirectory() as d:
            fi, fo = os.path.join(d, "i"), os.path.join(d, "o")
            with open(fi, "wb") as f:
                f.write(struct.pack("3i", n, K, m))
                for a in (pts, pairs, lists, fives, Rs):
                    f.write(np.ascontiguousarray(a).tobytes())
            subprocess.run([tool, fi, fo], check=True)
            raw = np.frombuffer(open(fo, "rb").read(), np.float64)
        o = 0

        def take(c):
            nonlocal o
            v = raw[o:o + c].copy()
            o += c
            return v

        g = dict(pts=pts, pairs=pairs, lists=lists, fives=fives, Rs=Rs, R2=take(K * 9).reshape(K, 9), Rn=take(K * 9).reshape(K, 9),
                 t2=take(K * 3).reshape(K, 3))
        e = take(K * 24).reshape(K, 24)
        g.update(eigR=e[:, :9], eigD=e[:, 9:12], eigV=e[:, 12:21], eigT=e[:, 21:24], err_rot=take(n), err_nomot=take(n), err_trans=take(n))
        assert o == len(raw)
        for k2, v in g.items():
            out[f"{name}_{k2}"] = v
        print(f"degen math {name}: twopt_rot det {np.linalg.det(g['R2'][0].reshape(3, 3)):.6f}, rot errors < 5e-7: {(g['err_rot'] < 5e-7).sum()}")
    np.savez_compressed(os.path.join(HERE, "usac_degen_math.npz"), **out)
    print("usac_degen_math: ok", os.path.getsize(os.path.join(HERE, "usac_degen_math.npz")), "bytes")


def eigen_order_case():
    """The ORDER of Eigen::EigenSolver<Matrix3d>'s eigenvalues (the Eigen the reference vendors, oracle/_ref/eigen_svd3 eig) on symmetric
    matrices of the kind OpenGV's eigensolver decomposes -- sum of outer products of nearly coplanar vectors: one small eigenvalue, down
    to exactly singular -- and on indefinite symmetric ones.  OpenGV takes column 0 as the translation."""
    import struct
    import subprocess
    import tempfile

    tool = os.path.join(ROOT, "oracle", "_ref", "eigen_svd3")
    rng = np.random.default_rng(20260901)
    Ms = []
    for it in range(1500):
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        noise = (1e-1, 1e-3, 1e-6, 0.5, 1e-9, 0.0)[it % 6]
        M = np.zeros((3, 3))
        for _ in range(3 if it % 7 == 0 else 5):
            v = rng.uniform(-1, 1, 3)
            v = v - (v @ t) * t + noise * rng.uniform(-1, 1, 3)
            v *= 1.0 if it % 5 == 0 else 0.05
            M += np.outer(v, v)
        if it % 11 == 0:
            A = rng.uniform(-1, 1, (3, 3))
            M = A + A.T
        Ms.append(M)
    Ms = np.array(Ms)
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "i"), os.path.join(d, "o")
        with open(fi, "wb") as f:
            f.write(struct.pack("i", len(Ms)))
            f.write(Ms.tobytes())
        subprocess.run([tool, fi, fo, "eig"], check=True)
        D = np.frombuffer(open(fo, "rb").read(), np.float64).reshape(-1, 3).copy()
    first_is_smallest = int((np.argmin(D, axis=1) == 0).sum())
    np.savez_compressed(os.path.join(HERE, "eigen_order3.npz"), M=Ms, D=D)
    print(f"eigen_order3: ok {len(Ms)} matrices, smallest eigenvalue at position 0 in {first_is_smallest}")


# ---- the `live` tests' inputs and the reference-built checkers' outputs on them (tests/golden/ref_live.npz) ---------------------------
def live_svd_inputs():
    return np.random.default_rng(5).standard_normal((300, 3, 3))


def live_nms_inputs():
    return synth.orb_pair(300, 500, seed=77)


def live_usac_trials():
    """(trial, n, frac, seed) of the six USAC scenes"""
    rng = np.random.default_rng(77)
    for trial in range(6):
        yield trial, int(rng.integers(60, 1500)), float(rng.uniform(0.35, 0.9)), int(rng.integers(1, 10 ** 6))


def live_usac_run(trial, n, frac, seed):
    """oracle/_ref/usac_ref on one scene of live_usac_trials (PROSAC on odd trials)"""
    import usac_ref_tool

    p1, p2, th, truth, order = usac_scene(n, frac, seed)
    return usac_ref_tool.run(p1, p2, th, 1000 + trial, sorted_idx=order if trial % 2 else None, solver_oracle=True)


def run_eigen_svd3(Ms):
    """oracle/_ref/eigen_svd3 -> (len(Ms), 21) float64: singular values, U, V (row-major)"""
    import struct

    tool = oracle_lib.ref_tool("eigen_svd3")
    assert tool, "build oracle/_ref first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "i.bin"), os.path.join(d, "o.bin")
        open(fi, "wb").write(struct.pack("i", len(Ms)) + np.ascontiguousarray(Ms).tobytes())
        subprocess.run([tool, fi, fo], check=True)
        return np.fromfile(fo).reshape(-1, 21)


def ref_live_case():
    """What the reference-built checkers return on the inputs of the three `live` tests (test_oracle_arrsac, test_oracle_matching,
    test_oracle_usac), so that those tests run where oracle/_ref cannot be built; where it can, they run the tools again and require
    exactly these outputs."""
    out = {"svd": run_eigen_svd3(live_svd_inputs())}
    out["nms_idx"], out["nms_dist"] = run_nmslib("hamming", *live_nms_inputs())
    for trial, n, frac, seed in live_usac_trials():
        r = live_usac_run(trial, n, frac, seed)
        for k in ("events", "final", "flags", "pool"):
            out[f"usac{trial}_{k}"] = r[k]
    np.savez_compressed(os.path.join(HERE, "ref_live.npz"), **out)
    print("ref_live: ok", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("all", "ref_live"):
        ref_live_case()
    if what in ("all", "usac"):
        usac_case()
    if what in ("all", "usac_stewenius"):
        usac_stewenius_case()
    if what in ("all", "usac_refine"):
        usac_refine_case()
    if what in ("all", "degen"):
        degen_math_case()
    if what in ("all", "eigen"):
        eigen_svd_case()
    if what in ("all", "eigenorder"):
        eigen_order_case()
    if what in ("all", "arrsac"):
        arrsac_case()
    if what in ("all", "nms"):
        nms_wrapper_case()
    if what in ("all", "matching"):
        main()
    if what in ("all", "pose"):
        fivept_case()
    if what in ("all", "l2"):
        l2_case()
    if what in ("all", "ransac"):
        ransac_case()
    if what in ("all", "cheirality"):
        cheirality_case()
    if what in ("all", "coeff"):
        coeff_case()
