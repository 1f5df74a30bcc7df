"""Device fit of the CLaSS proposal Q(z) (cpg.gmm.DiagGaussianMixture) against scikit-learn: prints ONE JSON line.

Per N in --sizes (D = 100, K = 100, f32, clustered data): device time per phase (k-means++ seeding, Lloyd, initial M-step, EM) from
CUDA events around each phase, the EM and Lloyd time per pass, and the achieved GB/s on design bytes (X read once per pass) against
the 8 TB/s spec and the 6.3 TB/s measured copy rate.  Per-iteration times come from events on the stream, so they include the
launch gap after each iteration's scalar read-back.  scikit-learn's GaussianMixture(diag) on the same data is timed at the sizes
in --sklearn-sizes, with the host core count.  Run it on the GPU under `timeout -k 10 <s>`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "controlled-peptide-generation_amd"))

SPEC_TBS, COPY_TBS = 8.0, 6.3


def blobs(n, D, K, seed):
    rs = np.random.RandomState(seed)
    centers = rs.randn(K, D) * 2.0
    lab = rs.randint(0, K, size=n)
    return (centers[lab] + rs.randn(n, D).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000,1000000")
    ap.add_argument("--sklearn-sizes", default="200000")
    ap.add_argument("--D", type=int, default=100)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2, help="device fits per size; the last is reported (the first warms up)")
    a = ap.parse_args()
    import torch
    from cpg.gmm import DiagGaussianMixture
    out = {"tool": "gmm_fit_bench", "D": a.D, "K": a.K, "dtype": "float32", "spec_TBps": SPEC_TBS, "copy_TBps": COPY_TBS,
           "host_cores": os.cpu_count(), "runs": []}
    sk_sizes = {int(s) for s in a.sklearn_sizes.split(",") if s}
    for n in (int(s) for s in a.sizes.split(",")):
        X = blobs(n, a.D, a.K, 7)
        x = torch.from_numpy(X).cuda()
        xbytes = X.nbytes
        for _ in range(a.reps):
            m = DiagGaussianMixture(n_components=a.K, random_state=0, timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        t = m.timings_
        em = t["em_iter_ms"]
        em_pass = float(np.median(em)) if em else float("nan")
        lloyd_pass = t["lloyd"] / max(m._kmeans_n_iter + 1, 1)   # + the final labelling pass when not strictly converged (upper bound)
        r = {"n": n, "X_MB": xbytes / 1e6, "fit_wall_s": wall, "seeding_ms": t["seeding"], "lloyd_ms": t["lloyd"],
             "lloyd_iters": m._kmeans_n_iter, "lloyd_pass_ms": lloyd_pass, "init_mstep_ms": t["init"], "em_ms": t["em"],
             "em_iters": m.n_iter_, "em_pass_ms_median": em_pass, "converged": bool(m.converged_),
             "em_pass_GBps": xbytes / (em_pass * 1e-3) / 1e9, "lloyd_pass_GBps": xbytes / (lloyd_pass * 1e-3) / 1e9}
        r["em_frac_spec"] = r["em_pass_GBps"] / (SPEC_TBS * 1e3)
        r["em_frac_copy"] = r["em_pass_GBps"] / (COPY_TBS * 1e3)
        r["lloyd_frac_spec"] = r["lloyd_pass_GBps"] / (SPEC_TBS * 1e3)
        if n in sk_sizes:
            from sklearn.mixture import GaussianMixture
            t0 = time.perf_counter()
            ref = GaussianMixture(n_components=a.K, covariance_type="diag", random_state=0).fit(X)
            r["sklearn_fit_s"] = time.perf_counter() - t0
            r["sklearn_iters"] = int(ref.n_iter_)
            r["speedup_vs_sklearn"] = r["sklearn_fit_s"] / wall
            r["same_n_iter_as_sklearn"] = int(ref.n_iter_) == int(m.n_iter_)
        out["runs"].append(r)
        del x
    print(json.dumps(out))


if __name__ == "__main__":
    main()
