"""Per-kernel throughput of the gfx950 hot path (diagnostic companion of bench.py).

Prints one JSON object per kernel: time per launch (HIP events on the launch stream),
pairs/s, algorithmic flop/s and transcendental/s against the probed VALU peaks
(libdifficp_microbench.so), algorithmic HBM GB/s.

    python bench_kernels.py [--quick] [--only KRED,ODE_FWD,...]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from difficp_amd import _lib  # noqa: E402

# Algorithmic cost per pair for D = 3 (FMA = 2 flop; exp2 = 1 transcendental "T").
# Counted from the pair operators in diff-icp_amd/csrc/lddmm_ops.hpp / gmm.hip.
FLOPS_PER_PAIR = {
    "KRED": 15, "GRADK": 15, "GENDK": 21,
    "ODE_FWD": 33,            # v, Z, G with DIV (eta = 0)
    "ODE_BWD": 80,            # fused VJP (eta = 0)
    "GMM_ESTEP": 2 * 13 + 12,  # two sweeps (max, then exp + 6 weighted sums)
    "GMM_MSTEP": 2 * 13 + 6,
    "GMM_TARGETS": 30,
    "GMM_ESTEP_NOSTATS": 12,  # 3 sub + 4 fma + the sum of the exps (+ 1 exp)
    "GMM_ASSIGN_K1": 13, "GMM_ASSIGN_K4": 13,   # 3 sub + mul + 3 fma, compare / select; no exp
    # soft transfer (csrc/carry.hip): 3 sub + mul + 3 fma, the shift, the sum of the exps (+ 1 exp)
    # and one fma per channel
    "GMM_CARRY_F1": 14 + 2 * 1, "GMM_CARRY_F4": 14 + 2 * 4, "GMM_CARRY_F16": 14 + 2 * 16,
    # RKHS Gram entries (csrc/gram.hip): 3 sub + mul + 2 fma, mul + 2 fma, the exponent's mul,
    # the fma into the tile sum (+ 1 exp); the composed route is one KRed per pair (15)
    "RKHS_GRAM": 17, "GRAM_BY_KRED": 15,
    "ODE_EXT_FWD": 22,        # v and the divergence row (eta = 0): 3 sub + mul + 7 fma
    "EXT_JAC": 35, "EXT_JAC_STEP": 35,   # v and the D x D gradient (eta = 0): 3 sub + 4 mul + 3 add + 12 fma
    # tangent-linear pass (csrc/tlm.hip): 66 per self pair and 32 per carried pair, M = N: 49 on
    # average; the central difference pays 2 x (33 + 22) per such pair of pairs
    "TLM": 49, "TLM_BY_DIFFERENCE": 55,
    # second-order pass (csrc/hvp.hip), without and with the cost terms; the VJP beside it
    "HVP": 133, "HVP_COST": 194, "HVP_VJP": 80,
}
# HBM bytes per launch (algorithmic: each input read once, each output written once).


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def probe_peaks():
    path = os.path.join(ROOT, "diff-icp_amd", "libdifficp_microbench.so")
    mb = ctypes.CDLL(path)
    mb.dicp_mb_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.c_void_p]
    chains = mb.dicp_mb_chains()
    out = torch.zeros(256, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    blocks, iters = 256 * 8 * 4, 4096
    res = {}
    for kind, name, mult in ((0, "exp2_per_s", 1), (1, "fma_flops", 2), (2, "pk_fma_flops", 4),
                             (3, "dpp_wave_rol_add_per_s", 1), (4, "dpp_row_ror_add_per_s", 1),
                             (5, "fma_flops_with_1exp_per_8fma", 2)):
        t = timed(lambda: mb.dicp_mb_launch(kind, blocks, iters, ctypes.c_void_p(out.data_ptr()), st),
                  warm=2, reps=5)
        res[name] = blocks * 256 * iters * chains * mult / t
    # SIMD cycles per wave64 instruction at the nominal 2.4 GHz, 1024 SIMDs
    res["cycles_per_wave_instr"] = {k: 1024 * 2.4e9 * 64 * m / res[k] for k, m in (
        ("exp2_per_s", 1), ("fma_flops", 2), ("dpp_wave_rol_add_per_s", 1),
        ("dpp_row_ror_add_per_s", 1))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    only = set(args.only.split(",")) if args.only else None
    results = []

    peaks = probe_peaks()
    print(json.dumps({"peaks": peaks}), flush=True)
    results.append({"peaks": peaks})

    def rep(name, t, pairs, bytes_, extra=None):
        fl = FLOPS_PER_PAIR.get(name.split("@")[0], 0) * pairs
        r = {"kernel": name, "ms": t * 1e3, "Gpairs_per_s": pairs / t / 1e9,
             "TFLOPs": fl / t / 1e12, "Texp_per_s": pairs / t / 1e12,
             "frac_fp32_peak": fl / t / peaks["pk_fma_flops"],
             "frac_exp_peak": pairs / t / peaks["exp2_per_s"],
             "alg_GBps": bytes_ / t / 1e9, "splits": None}
        if extra:
            r.update(extra)
        print(json.dumps(r), flush=True)
        results.append(r)

    D = 3
    n_big = 20000 if args.quick else 100000
    if only is None or "KRED" in only:
        x = torch.rand(n_big, D, device=dev)
        b = torch.randn(n_big, D, device=dev)
        t = timed(lambda: _lib.gauss_red(_lib.KRED, x, x, 0.1, b=b))
        rep(f"KRED@{n_big}x{n_big}", t, n_big * n_big, 4 * (3 * n_big + 6 * n_big + 3 * n_big),
            {"splits": _lib.num_splits(_lib.WS_RED, n_big, n_big)})
    for M in ([20000] if args.quick else [20000, 50000, 200000]):
        if only is not None and "ODE" not in only:
            break
        q = torch.rand(M, D, device=dev)
        p = 0.01 * torch.randn(M, D, device=dev)
        t = timed(lambda: _lib.ode_self_fwd(q, p, 0.1, 0.0, True), reps=5)
        rep(f"ODE_FWD@{M}", t, M * M, 4 * (6 * M + 6 * M + 7 * M))
        a = torch.randn(M, D, device=dev)
        bm = torch.randn(M, D, device=dev)
        gd = torch.ones(1, device=dev)
        t = timed(lambda: _lib.ode_self_bwd(q, p, a, bm, gd, 0.1, 0.0), reps=5)
        rep(f"ODE_BWD@{M}", t, M * M, 4 * (12 * M + 12 * M + 6 * M))
    if only is None or "GMM" in only:
        for (N, C) in ([(50000, 50000)] if args.quick else [(50000, 50000), (640000, 512), (200000, 200000)]):
            X = torch.rand(N, D, device=dev)
            mu = torch.rand(C, D, device=dev)
            w2 = torch.zeros(C, device=dev)
            mu2 = (mu * mu).sum(-1)
            t = timed(lambda: _lib.gmm_estep(X, mu, w2, mu2, 0.05, 0.0, True), reps=5)
            rep(f"GMM_ESTEP@{N}x{C}", t, N * C, 4 * (3 * N + 5 * C + 9 * N))
            T, T2, _ = _lib.gmm_estep(X, mu, w2, mu2, 0.05, 0.0, False)
            t = timed(lambda: _lib.gmm_mstep(X, T2, mu, w2, 0.05), reps=5)
            rep(f"GMM_MSTEP@{N}x{C}", t, N * C, 4 * (4 * N + 4 * C + 4 * C))
            t = timed(lambda: _lib.gmm_targets(X, T2, mu, w2, 0.05, mu, w2), reps=5)
            rep(f"GMM_TARGETS@{N}x{C}", t, N * C, 4 * (4 * N + 9 * C + 7 * N))
    if only is None or "ASSIGN" in only:
        # the top-k correspondence pass next to its yardstick, the stats-less E-step (the same
        # pair count plus an exp), 100 back-to-back launches each, alternated three times so the
        # lines show the spread; then the whole GaussianMixtureUnif.assign call (that E-step +
        # the top-k pass + O(N k) torch)
        from difficp_amd.core.GMM import GaussianMixtureUnif
        N = C = n_big
        X = torch.rand(N, D, device=dev)
        mu = torch.rand(C, D, device=dev)
        G = GaussianMixtureUnif(mu, sigma=0.05, spec={"device": dev, "dtype": torch.float32})
        _, w2, mu2 = G._columns(G.mu, G.w)
        nbytes = 4 * (4 * N + 4 * C)
        for _ in range(3):
            t = timed(lambda: _lib.gmm_estep(X, mu, w2, mu2, 0.05, 0.0, False), reps=100)
            rep(f"GMM_ESTEP_NOSTATS@{N}x{C}", t, N * C, nbytes + 8 * N,
                {"splits": _lib.num_splits(_lib.WS_GMM_ESTEP, N, C)})
            for K in (1, 4):
                t = timed(lambda: _lib.gmm_assign(X, mu, w2, 0.05, K), reps=100)
                rep(f"GMM_ASSIGN_K{K}@{N}x{C}", t, N * C, nbytes + 8 * N * K,
                    {"splits": _lib.num_splits(_lib.WS_GMM_ASSIGN, N, C), "Texp_per_s": 0.0,
                     "frac_exp_peak": 0.0})
        for K in (1, 4):
            t = timed(lambda: G.assign(X, k=K), reps=100)
            rep(f"API_ASSIGN_K{K}@{N}x{C}", t, N * C, 2 * nbytes + 8 * N * (K + 1))
    if only is None or "CARRY" in only:
        # the soft transfer next to its yardstick, the stats-less E-step at the same shape (the
        # same pair count and one exp per pair), in the manner of ASSIGN: 100 back-to-back
        # launches each, alternated three times; the 100k square, then the atlas shapes (carry:
        # points x components; pool: components x points, which exercises the column split)
        for (M, N, Fs) in [(n_big, n_big, (1, 4, 16)), (20000, 512, (1, 16)), (512, 640000, (1, 16))]:
            rows = torch.rand(M, D, device=dev)
            cols = torch.rand(N, D, device=dev)
            bias = torch.randn(N, device=dev)
            c2 = (cols * cols).sum(-1)
            feats = {F: torch.randn(N, F, device=dev) for F in Fs}
            nbytes = 4 * (4 * M + 4 * N)
            for _ in range(3):
                t = timed(lambda: _lib.gmm_estep(rows, cols, bias, c2, 0.05, 0.0, False), reps=100)
                rep(f"GMM_ESTEP_NOSTATS@{M}x{N}", t, M * N, nbytes + 8 * M,
                    {"splits": _lib.num_splits(_lib.WS_GMM_ESTEP, M, N)})
                for F in Fs:
                    t = timed(lambda: _lib.gmm_carry(rows, cols, bias, feats[F], 0.05), reps=100)
                    rep(f"GMM_CARRY_F{F}@{M}x{N}", t, M * N, nbytes + 4 * (N * F + M * (F + 1)),
                        {"splits": _lib.num_splits(_lib.WS_GMM_CARRY, M, N)})
    if only is None or "GRAM" in only:
        # all K (K + 1) / 2 inner products of an atlas' fields: one rkhs_gram call next to the
        # route the reductions allow, (p_a * KRed(q_a, q_b, p_b)).sum() per pair (float64 sum of
        # the float32 rows, no host read), in the same process, alternated three times
        K, M = (8, 20000) if args.quick else (32, 20000)
        qs = [torch.rand(M, D, device=dev) for _ in range(K)]
        ps = [0.01 * torch.randn(M, D, device=dev) for _ in range(K)]
        q, p = torch.cat(qs), torch.cat(ps)
        offsets = [k * M for k in range(K + 1)]
        pairs = torch.triu_indices(K, K).t().contiguous()
        npairs = pairs.shape[0]

        def composed():
            out = torch.empty(npairs, device=dev, dtype=torch.float64)
            for n, (a, b) in enumerate(pairs.tolist()):
                out[n] = (ps[a].double() * _lib.gauss_red(_lib.KRED, qs[a], qs[b], 0.1, b=ps[b]).double()).sum()
            return out

        nbytes = 4 * 2 * D * 2 * M * npairs
        for _ in range(3):
            t = timed(lambda: _lib.rkhs_gram(q, p, offsets, pairs, 0.1), warm=1, reps=3)
            rep(f"RKHS_GRAM@{K}x{M}", t, npairs * M * M, nbytes + 8 * npairs,
                {"pairs": npairs, "splits": _lib.num_splits(_lib.WS_RKHS_GRAM, M, npairs)})
            t = timed(composed, warm=1, reps=1)
            rep(f"GRAM_BY_KRED@{K}x{M}", t, npairs * M * M, nbytes + 4 * D * M * npairs, {"pairs": npairs})
        g1, g2 = _lib.rkhs_gram(q, p, offsets, pairs, 0.1), composed()
        print(json.dumps({"gram_vs_composed_max_rel": float(((g1 - g2).abs() / g1.abs().max()).max())}),
              flush=True)
    if only is None or "EXT_JAC" in only:
        # the velocity-gradient pass (csrc/ext_jac.hip) next to its yardstick, the external-point
        # forward with the divergence row, at the same N x M: back-to-back launches, alternated
        # three times so the lines show the spread -- on the default dispatch (the forward may take
        # the centred expansion) and with red_alg 0 / ext_alg 1 (both on the packed row skeleton);
        # then a 10-step flow_jacobian next to apply
        from difficp_amd.core.LDDMM import LDDMMModel
        from difficp_amd.core.registrations import LDDMMRegistration
        for (N, M) in [(n_big, n_big), (n_big, n_big // 5)]:
            x = torch.rand(N, D, device=dev)
            q = torch.rand(M, D, device=dev)
            p = 0.01 * torch.randn(M, D, device=dev)
            G = 0.1 * torch.randn(N, D, D, device=dev)
            nb = 4 * (3 * N + 6 * M)
            for mode, opts in (("default", {}), ("packed", {"red_alg": 0, "ext_alg": 1})):
                old = {k: _lib.get_option(k) for k in opts}
                for k, v in opts.items():
                    _lib.set_option(k, v)
                try:
                    for _ in range(3):
                        for eta in (0.0, 2e-3):
                            ex = {"dispatch": mode, "eta": eta}
                            t = timed(lambda: _lib.ode_ext_fwd(x, q, p, 0.1, eta, True), reps=50)
                            rep(f"ODE_EXT_FWD@{N}x{M}", t, N * M, nb + 16 * N,
                                dict(ex, splits=_lib.num_splits(_lib.WS_ODE_EXT_FWD, M, N)))
                            t = timed(lambda: _lib.ode_ext_jac(x, q, p, 0.1, eta), reps=50)
                            rep(f"EXT_JAC@{N}x{M}", t, N * M, nb + 48 * N,
                                dict(ex, splits=_lib.num_splits(_lib.WS_ODE_EXT_JAC, M, N)))
                    t = timed(lambda: _lib.ext_jac_step(x, G, q, p, 0.1, 0.0, 0.1), reps=50)
                    rep(f"EXT_JAC_STEP@{N}x{M}", t, N * M, nb + 84 * N, {"dispatch": mode, "eta": 0.0})
                finally:
                    for k, v in old.items():
                        _lib.set_option(k, v)
        N = M = n_big
        LM = LDDMMModel(sigma=0.1, D=D, lambd=100.0, version="hybrid", scheme="Euler", nt=10,
                        spec={"device": dev, "dtype": torch.float32})
        reg = LDDMMRegistration(LM, torch.rand(M, D, device=dev), 0.001 * torch.randn(M, D, device=dev))
        X = torch.rand(N, D, device=dev)
        sh = reg.shoot(None)
        for _ in range(3):
            LM.shoot_cache.clear()
            t = timed(lambda: (LM.shoot_cache.clear(), reg.apply(X)), warm=1, reps=5)
            rep(f"API_APPLY@{N}x{M}", t, 10 * N * M, 0)
            t = timed(lambda: reg.apply_with_jacobian(X), warm=1, reps=5)
            rep(f"API_APPLY_WITH_JACOBIAN@{N}x{M}", t, 10 * N * M, 0)
            t = timed(lambda: LM.flow_jacobian(reg.q0, reg.a0, X, shoot=sh), warm=1, reps=5)
            rep(f"API_FLOW_JACOBIAN_GIVEN_SHOOT@{N}x{M}", t, 10 * N * M, 0)
    if only is None or "TLM" in only:
        # one tangent-linear pass (self + carried part, csrc/tlm.hip) for L directions next to what
        # a central difference pays per direction on the forward kernels -- two self forwards and
        # two external-point forwards at the displaced states -- in the same process, alternated
        # three times; then the pass with 1 and 2 row pairs per thread forced (option pk_rp)
        for M in ([20000] if args.quick else [20000, 100000]):
            N = M
            q, x = torch.rand(M, D, device=dev), torch.rand(N, D, device=dev)
            p = 0.01 * torch.randn(M, D, device=dev)
            for L in (1, 4):
                dq, dp = 0.1 * torch.randn(L, M, D, device=dev), 0.01 * torch.randn(L, M, D, device=dev)
                dx = 0.1 * torch.randn(L, N, D, device=dev)
                h = 1e-3
                states = [(q + s * h * dq[l], p + s * h * dp[l], x + s * h * dx[l])
                          for l in range(L) for s in (1.0, -1.0)]

                def difference():
                    for qs, ps, xs in states:
                        _lib.ode_self_fwd(qs, ps, 0.1, 0.0, False)
                        _lib.ode_ext_fwd(xs, qs, ps, 0.1, 0.0, False)

                pairs = L * M * (M + N)
                nb = 4 * D * (2 * M + N + L * (4 * M + 2 * N))
                ex = {"L": L, "splits": _lib.num_splits(_lib.WS_ODE_TLM, M, N)}
                for _ in range(3):
                    t = timed(lambda: _lib.ode_tlm(q, p, dq, dp, 0.1, x, dx), reps=5)
                    rep(f"TLM@{N}x{M}", t, pairs, nb, ex)
                    t = timed(difference, reps=5)
                    rep(f"TLM_BY_DIFFERENCE@{N}x{M}", t, 2 * pairs, 2 * L * 4 * D * (5 * M + 2 * N), {"L": L})
                old = _lib.get_option("pk_rp")
                try:
                    for rp in (1, 2):
                        _lib.set_option("pk_rp", rp)
                        t = timed(lambda: _lib.ode_tlm(q, p, dq, dp, 0.1, x, dx), reps=5)
                        rep(f"TLM@{N}x{M}", t, pairs, nb, dict(ex, pk_rp=rp))
                finally:
                    _lib.set_option("pk_rp", old)
    if only is None or "HVP" in only:
        # one second-order pass (csrc/hvp.hip) for L directions, without and with the cost terms,
        # next to the L VJPs a stage of LDDMMModel.loss_hvp runs beside it; alternated three times
        for M in ([20000] if args.quick else [20000, 100000]):
            q, p = torch.rand(M, D, device=dev), 0.01 * torch.randn(M, D, device=dev)
            aq, ap = 0.1 * torch.randn(M, D, device=dev), 0.01 * torch.randn(M, D, device=dev)
            g = torch.ones(1, device=dev)
            for L in (1, 4):
                bq, bp = 0.1 * torch.randn(L, M, D, device=dev), 0.01 * torch.randn(L, M, D, device=dev)
                nb = 4 * D * M * (4 + 4 * L)
                ex = {"L": L, "splits": _lib.num_splits(_lib.WS_ODE_HVP, M, M)}
                for _ in range(3):
                    t = timed(lambda: _lib.ode_hvp(q, p, aq, ap, bq, bp, 0.1), reps=5)
                    rep(f"HVP@{M}x{M}", t, L * M * M, nb, ex)
                    t = timed(lambda: _lib.ode_hvp(q, p, aq, ap, bq, bp, 0.1, g), reps=5)
                    rep(f"HVP_COST@{M}x{M}", t, L * M * M, nb, ex)
                    t = timed(lambda: [_lib.ode_self_bwd(q, p, bq[l], bp[l], None, 0.1, 0.0) for l in range(L)],
                              reps=5)
                    rep(f"HVP_VJP@{M}x{M}", t, L * M * M, L * 4 * M * 6 * D, {"L": L})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
