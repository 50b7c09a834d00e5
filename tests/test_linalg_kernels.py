"""The dense Newton-step factorisations and the wave primitives, routine by routine, against float64 numpy.

tests/linalg/linalg_probe.hip calls the product's routines (rg_kernel.h, rb_kernel.h) as they are, one workgroup per matrix; every check
runs on the host emulation of the wavefront (`emul`, the CPU suite) and on the gfx950 build (`gpu`, -m gpu): the device branches of the
collectives, the matrix pipe and v_rcp / v_rsq are only exercised by the second.

Rules (eps = 2^-24, one constant C for all routines; none of them depends on a measured number):
  backward error   |H x - g|_inf / (|H|_inf |x|_inf + |g|_inf)   <= C n eps
  forward error    |x - x*|_inf / |x*|_inf                       <= C n eps cond(S H S),  S = diag(H)^-1/2   (van der Sluis)
  factor           |L L' - H|_max / |H|_max                      <= C n eps
  inverse factor   |W' H W - I|_max                               <= C n eps cond(H)
  Woodbury         error <= 10 x (error of a fresh factorisation of H_new by the same routine) x A + C n eps |x*|_inf,
                   A = max(1, 1 / rho) over the rows that leave, rho = 1 - D j' inv(H_old) j (the ratio the routine's own singularity test bounds by 1e-4)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDIR = os.path.join(ROOT, "tests", "linalg")
EPS = 2.0 ** -24
C = 4.0                       # the one constant of the error rules above
BAD_FACTOR = 16               # RG_STATUS_BAD_FACTOR (rg_types.h)


class Probe:
    def __init__(self, path, tier):
        self.tier = tier
        L = self.L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.lp_rg.restype = ctypes.c_int
        L.lp_rb.restype = ctypes.c_int
        L.lp_prim.restype = ctypes.c_int
        lim = np.zeros(8, np.int32)
        L.lp_rg_limits(lim.ctypes.data_as(vp))
        self.hwords, self.maxnvc, self.woodbury, self.maxsrow, self.maxten, self.maxcon, self.cpool, self.rgw = (int(v) for v in lim)
        L.lp_rb_limits(lim.ctypes.data_as(vp))
        self.rb_group = [int(v) for v in lim[:3]]

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def rg(self, op, Hs, gs, g2s=None, wood=None):
        """Hs: [B][n][n] (the lower triangle is what the work rows carry; the strict upper triangle is filled with NaN: never read),
        gs / g2s: [B][n].  Returns x, x2, work rows [B][n + 1][hs], status words, return values."""
        Hs = np.asarray(Hs, np.float64); B, n = Hs.shape[0], Hs.shape[1]
        hs = (n + 3) // 4 * 4
        work = np.zeros((B, n + 1, hs), np.float32)
        for b in range(B):
            h = np.tril(Hs[b]).astype(np.float32)
            h[np.triu_indices(n, 1)] = np.nan
            work[b, :n, :n] = h
            work[b, n, :n] = gs[b]
        g2 = None if g2s is None else np.ascontiguousarray(np.asarray(g2s, np.float32))
        x, x2 = np.zeros((B, n), np.float32), np.zeros((B, n), np.float32)
        hout, st = np.zeros_like(work), np.zeros((B, 2), np.uint32)
        w = wood or {}
        ns, ncon = w.get("ns", 0), w.get("ncon", 0)
        arr = lambda k, t: None if k not in w else np.ascontiguousarray(np.asarray(w[k], t))
        keep = [arr(k, t) for k, t in (("sdesc", np.int32), ("sD", np.float32), ("squad", np.int32), ("pquad", np.int32), ("cdim", np.int32), ("cnnz", np.int32),
                                        ("coff", np.int32), ("cidx", np.int32), ("cD", np.float32), ("cmu", np.float32), ("cpool", np.float32), ("tcdof", np.int32), ("tenJ", np.float32))]
        rc = self.L.lp_rg(op, n, B, self._p(work), self._p(g2), ns, *[self._p(keep[0]), self._p(keep[1]), self._p(keep[2])], ncon,
                          *[self._p(k) for k in keep[3:]], self._p(x), self._p(x2), self._p(hout), self._p(st))
        assert rc == 0, "lp_rg failed (%d)" % rc
        return x.astype(np.float64), x2.astype(np.float64), hout, st[:, 0], st[:, 1]

    def rb(self, cfg, op, As, gs, perm=None):
        As = np.asarray(As, np.float64); B, n = As.shape[0], As.shape[1]
        perm = np.arange(n, dtype=np.int32) if perm is None else np.asarray(perm, np.int32)
        il = np.tril_indices(n)
        packed = np.ascontiguousarray(np.stack([a[il] for a in As]).astype(np.float32))   # row-major packed lower triangle = RB_TRI order
        # right-hand side by dof: group slot l holds dof perm[l]
        g = np.zeros((B, n), np.float32); g[:, perm] = np.asarray(gs, np.float32)
        x, aout, sc, ret = np.zeros((B, n), np.float32), np.zeros_like(packed), np.zeros((B, n), np.float32), np.zeros(B, np.uint32)
        rc = self.L.lp_rb(cfg, op, n, B, self._p(packed), self._p(g), self._p(perm), self._p(x), self._p(aout), self._p(sc), self._p(ret))
        assert rc == 0, "lp_rb failed (%d)" % rc
        xs = x[:, perm].astype(np.float64)     # back to group order
        Ls = np.zeros((B, n, n))
        for b in range(B):
            Ls[b][il] = aout[b]
        return xs, Ls, sc.astype(np.float64), ret

    def prim(self, v, u, iv, ix, fa=None, fb=None, fx=None):
        K = 0 if fa is None else len(fa)
        fa = np.zeros((1, 64), np.float32) if fa is None else np.ascontiguousarray(fa, np.float32)
        fb = np.zeros((1, 64), np.float32) if fb is None else np.ascontiguousarray(fb, np.float32)
        fx = np.zeros(1, np.float32) if fx is None else np.ascontiguousarray(fx, np.float32)
        nf = 0 if fx is None else len(fx)
        out, iout, fo = np.zeros((64, 90), np.float32), np.zeros((64, 6), np.int32), np.zeros((max(nf, 1), 3), np.float32)
        args = [np.ascontiguousarray(v, np.float32), np.ascontiguousarray(u, np.float32), np.ascontiguousarray(iv, np.int32), np.ascontiguousarray(ix, np.int32)]
        rc = self.L.lp_prim(*[self._p(a) for a in args], K, self._p(fa), self._p(fb), nf, self._p(fx), self._p(out), self._p(iout), self._p(fo))
        assert rc == 0
        return out, iout, fo[:nf]


_probes = {}


@pytest.fixture(scope="module", params=["emul", pytest.param("gpu", marks=pytest.mark.gpu)])
def probe(request):
    tier = request.param
    if tier not in _probes:
        lib = "liblinalg_probe_emul.so" if tier == "emul" else "liblinalg_probe.so"
        subprocess.check_call(["make", "-C", LDIR, "-s", lib])
        _probes[tier] = Probe(os.path.join(LDIR, lib), tier)
    return _probes[tier]


# ------------------------------------------------------------------------------------------------- matrix families (fixed seeds)
def fam_cond(n, cond, seed):
    """(a) Q diag(lambda) Q' with eigenvalues log-spaced over `cond`."""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(n, n))
    lam = np.logspace(0, -np.log10(cond), n) if n > 1 else np.ones(1)
    return as_f32((Q * lam) @ Q.T)


def fam_structured(n, seed, dmax=1e6, mmin=1e-3):
    """(b) M + J' D J, what the Newton step sees: masses across mmin .. 1e2; single-dof rows (limits, dof friction) with weights up to dmax,
    multi-dof rows (contacts, tendons) whose Jacobian entries scale with the dofs' inertia, weights up to 1e2."""
    rng = np.random.RandomState(seed)
    mass = np.logspace(np.log10(mmin), 2, n)[rng.permutation(n)]
    R = rng.randn(n, n) / np.sqrt(n)
    sm = np.sqrt(mass)
    M = sm[:, None] * (np.eye(n) + 0.3 * R @ R.T) * sm[None, :]
    k1, k2 = max(1, n // 3), max(1, n // 3)
    J = np.zeros((k1 + k2, n))
    J[np.arange(k1), rng.choice(n, k1, replace=False)] = np.where(rng.rand(k1) < 0.5, 1.0, -1.0)
    for r in range(k1, k1 + k2):
        cols = rng.choice(n, size=min(n, 4), replace=False)
        J[r, cols] = rng.randn(len(cols)) * sm[cols]
    D = np.concatenate([np.logspace(0, np.log10(dmax), k1), np.logspace(0, 2, k2)])
    return as_f32(M + J.T @ (D[:, None] * J))


def fam_diag(n, seed):
    """(c) identity (seed 0) and a diagonal with entries across 1e-3 .. 1e3."""
    if seed == 0:
        return np.eye(n)
    rng = np.random.RandomState(seed)
    return as_f32(np.diag(np.logspace(-3, 3, n)[rng.permutation(n)]))


def fam_fail(n, kind, seed=0):
    """(d) inputs a factorisation must refuse: indefinite, singular (exactly, in fp32 arithmetic), a NaN entry, a pivot at the 1e-30 clamp."""
    H = fam_cond(n, 10.0, seed + 77)
    if kind == "indefinite":
        rng = np.random.RandomState(seed)
        Q, _ = np.linalg.qr(rng.randn(n, n))
        lam = np.linspace(1.0, 2.0, n); lam[n // 2] = -0.5
        H = as_f32((Q * lam) @ Q.T)
    elif kind == "singular":    # rows / columns i and i + 1 equal (powers of two): the pivot of i + 1 is exactly zero
        H = np.eye(n) * 4.0
        if n >= 2:
            i = n // 2 if n >= 3 else 0
            H[i, i] = H[i + 1, i + 1] = H[i + 1, i] = H[i, i + 1] = 4.0
        else:
            H[0, 0] = 0.0
    elif kind == "nan":
        H = H.copy(); i = n - 1; H[i, max(i - 1, 0)] = np.nan; H[max(i - 1, 0), i] = np.nan
    elif kind == "clamp":
        H = np.eye(n); H[n // 2, n // 2] = float(np.float32(1e-30))
    return H


def as_f32(H):
    H = 0.5 * (H + H.T)
    return H.astype(np.float32).astype(np.float64)


def rhs(n, seed):
    return np.random.RandomState(seed + 1000).randn(n).astype(np.float32).astype(np.float64)


def families(n):
    out = [("cond%.0e" % c, fam_cond(n, c, 10 * n + i)) for i, c in enumerate((1e1, 1e2, 1e4, 1e6))]
    out += [("structured%d" % s, fam_structured(n, 100 * n + s)) for s in range(2)]
    out += [("identity", fam_diag(n, 0)), ("diagonal", fam_diag(n, 5 + n))]
    return out


# ------------------------------------------------------------------------------------------------- error measures
def backward(H, x, g):
    r = H @ x - g
    return np.abs(r).max() / (np.abs(H).sum(1).max() * np.abs(x).max() + np.abs(g).max())


def scaled_cond(H):
    s = 1.0 / np.sqrt(np.diag(H))
    return np.linalg.cond(s[:, None] * H * s[None, :])


def forward(H, x, g):
    xs = np.linalg.solve(H, g)
    return np.abs(x - xs).max() / np.abs(xs).max()


def check_solve(name, H, x, g):
    n = len(g)
    be, fe, kc = backward(H, x, g), forward(H, x, g), scaled_cond(H)
    assert np.all(np.isfinite(x)), name
    assert be <= C * n * EPS, "%s: backward error %.3e > %.3e" % (name, be, C * n * EPS)
    assert fe <= C * n * EPS * kc, "%s: forward error %.3e > %.3e (cond(SHS) %.2e)" % (name, fe, C * n * EPS * kc, kc)
    return be, fe


def w_of(work, n):
    return work[:n, :n].astype(np.float64)


def check_inverse_factor(name, H, W):
    n = H.shape[0]
    assert np.all(W[np.tril_indices(n, -1)] == 0), "%s: W = inv(L') is not upper triangular (rg_cholinv_apply reads all of it)" % name
    e = np.abs(W.T @ H @ W - np.eye(n)).max()
    assert e <= C * n * EPS * np.linalg.cond(H), "%s: |W'HW - I| = %.3e" % (name, e)


# ------------------------------------------------------------------------------------------------- rg: register path, its reuse, the matrix pipe, the LDS path
@pytest.mark.parametrize("op", [0, 1], ids=["chol_inv_solve_n", "chol_mfma_n"])
@pytest.mark.parametrize("n", [24, 30])
def test_rg_register_solve_inverse_factor_and_reuse(probe, op, n):
    fams = families(n)
    Hs = np.stack([H for _, H in fams])
    gs = np.stack([rhs(n, i) for i in range(len(fams))])
    g2s = np.stack([rhs(n, 50 + i) for i in range(len(fams))])
    x, x2, work, st, _ = probe.rg(op, Hs, gs, g2s)
    for b, (name, H) in enumerate(fams):
        tag = "%s %s n=%d %s" % (probe.tier, ["reg", "mfma"][op], n, name)
        assert st[b] & BAD_FACTOR == 0, tag
        check_solve(tag, H, x[b], gs[b])
        check_inverse_factor(tag, H, w_of(work[b], n))
        check_solve(tag + " cholinv_apply", H, x2[b], g2s[b])


LDS_SIZES = [1, 2, 3, 4, 5, 24, 29, 30, 31, 32]


@pytest.mark.parametrize("n", LDS_SIZES)
@pytest.mark.parametrize("rhs_row", [True, False], ids=["rhs_row", "separate"])
def test_rg_lds_cholesky(probe, n, rhs_row):
    fams = families(n)
    Hs = np.stack([H for _, H in fams])
    gs = np.stack([rhs(n, i) for i in range(len(fams))])
    g2s = np.stack([rhs(n, 50 + i) for i in range(len(fams))])
    assert (n + 1) * ((n + 3) // 4 * 4) <= probe.hwords   # the right-hand-side row fits under every size tested
    x, x2, work, st, _ = probe.rg(2 if rhs_row else 3, Hs, gs, g2s)
    for b, (name, H) in enumerate(fams):
        tag = "%s lds n=%d %s %s" % (probe.tier, n, "rhs" if rhs_row else "sep", name)
        assert st[b] & BAD_FACTOR == 0, tag
        check_solve(tag, H, x[b], gs[b])
        L = np.tril(work[b, :n, :n].astype(np.float64))
        e = np.abs(L @ L.T - H).max() / np.abs(H).max()
        assert e <= C * n * EPS, "%s: |LL' - H| / |H| = %.3e" % (tag, e)
        if rhs_row:
            check_solve(tag + " chol_solve", H, x2[b], g2s[b])


ROUTES = {"reg24": (0, 24), "reg30": (0, 30), "mfma24": (1, 24), "mfma30": (1, 30), "lds5": (2, 5), "lds30": (2, 30), "lds30sep": (3, 30), "lds1sep": (3, 1)}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("kind", ["indefinite", "singular", "nan", "clamp"])
def test_rg_bad_factor_raised_exactly_on_failure_inputs(probe, route, kind):
    op, n = ROUTES[route]
    H = fam_fail(n, kind)
    ok_H = fam_cond(n, 1e3, 3)
    x, _, _, st, _ = probe.rg(op, np.stack([H, ok_H]), np.stack([rhs(n, 0), rhs(n, 1)]))
    assert st[0] & BAD_FACTOR, "%s %s %s: no RG_STATUS_BAD_FACTOR" % (probe.tier, route, kind)
    assert st[1] & BAD_FACTOR == 0, "%s %s: the flag leaked into a good workgroup" % (probe.tier, route)


# ------------------------------------------------------------------------------------------------- rg: Woodbury on the inverse factor
def _wood_setup(n, rows, seed, base=None):
    """rows: list of (kind, sign, enter) with kind in dof / tendon / pyramid.  Returns (H_old, H_new, table dict, [per-row (j, D, enter)])."""
    rng = np.random.RandomState(seed)
    Hb = fam_structured(n, seed, dmax=1e3, mmin=0.1) if base is None else base
    sdesc, sD, squad = [], [], []
    tcdof, tenJ = np.full(48, 255, np.int32), np.zeros(48, np.float32)
    ncon, cdim, cnnz, coff, cidx, cD, cmu, pquad = 0, [], [], [], [], [], [], []
    cpool = np.zeros(768, np.float32)
    changes, nten, off = [], 0, 0
    for kind, neg, enter, D in rows:
        j = np.zeros(n)
        if kind == "dof":
            d = int(rng.randint(n)); j[d] = 1.0
            sdesc.append(d | (31 << 6) | (neg << 11)); sD.append(D); squad.append(1 if enter else 2)
        elif kind == "tendon":
            t = nten; nten += 1
            ds = rng.choice(n, 3, replace=False); cs = rng.uniform(0.5, 1.5, 3).astype(np.float32)
            for e in range(3):
                tcdof[4 * t + e] = ds[e]; tenJ[4 * t + e] = cs[e]; j[ds[e]] += float(cs[e])
            sdesc.append((t << 6) | (neg << 11)); sD.append(D); squad.append(1 if enter else 2)
        else:   # a contact of condim 3 (pyramid rows 0..3) or 4 (rows 4, 5: spin); its changed pyramid row q = kind's index
            q = int(kind[-1]); c = ncon; ncon += 1
            dim, nb = (4, 4) if q >= 4 else (3, 3)
            nnz = 6; dofs = rng.choice(n, nnz, replace=False)
            B = rng.randn(nb, nnz).astype(np.float32); mu = [np.float32(0.8), np.float32(0.3)]
            cdim.append(dim); cnnz.append(nnz); coff.append(off); cD.append(D); cmu += mu
            cpool[off:off + nb * nnz] = B.ravel(); off += nb * nnz
            idx = np.zeros(14, np.int32); idx[:nnz] = dofs; cidx += list(idx)
            kb = q >> 1
            jr = B[0].astype(np.float64) + ((-1.0 if q & 1 else 1.0) * float(mu[kb >> 1])) * B[kb + 1].astype(np.float64)
            j[dofs] += jr
            pq = [0] * 6; pq[q] = 1 if enter else 2; pquad += pq
            neg = 0
        if kind in ("dof", "tendon") and neg:
            j = -j
        changes.append((j, float(np.float32(D)), enter))
    H_old, H_new = Hb.copy(), Hb.copy()
    for j, D, enter in changes:
        if enter:
            H_new += D * np.outer(j, j)
        else:
            H_old += D * np.outer(j, j)
    tab = dict(ns=len(sdesc), sdesc=sdesc or [0], sD=sD or [0.0], squad=squad or [0], ncon=ncon, pquad=pquad or [0], cdim=cdim or [0], cnnz=cnnz or [0],
               coff=coff or [0], cidx=cidx or [0], cD=cD or [0.0], cmu=cmu or [0.0], cpool=cpool, tcdof=tcdof, tenJ=tenJ)
    return as_f32(H_old), H_new, tab, changes


WOOD_CASES = {
    "1dof_enter": [("dof", 0, True, 50.0)],
    "1dof_leave": [("dof", 1, False, 5.0)],
    "2tendon_mixed": [("tendon", 0, True, 200.0), ("tendon", 1, False, 3.0)],
    "3pyr_mixed": [("pyr0", 0, True, 1e3), ("pyr3", 0, False, 2e2), ("pyr5", 0, True, 5e2)],
    "4all_kinds": [("dof", 0, True, 1e2), ("tendon", 0, False, 40.0), ("pyr1", 0, True, 3e2), ("pyr2", 0, False, 80.0)],
    "4leave": [("dof", 0, False, 20.0), ("dof", 1, False, 30.0), ("tendon", 1, False, 10.0), ("pyr4", 0, False, 60.0)],
}


@pytest.mark.parametrize("n", [24, 30])
@pytest.mark.parametrize("case", sorted(WOOD_CASES))
def test_rg_woodbury_against_fresh_factorisation(probe, n, case):
    rows = WOOD_CASES[case]
    assert len(rows) <= probe.woodbury
    H_old, H_new, tab, changes = _wood_setup(n, rows, seed=7 * n + len(case))
    g = rhs(n, 3)
    H_new32 = as_f32(H_new)
    _, xw, _, st, ret = probe.rg(4, H_old[None], rhs(n, 9)[None], g[None], wood=tab)
    assert st[0] & BAD_FACTOR == 0 and ret[0] == 1, "%s %s: Woodbury refused a well-conditioned update" % (probe.tier, case)
    xf, _, _, _, _ = probe.rg(0, H_new32[None], g[None])
    xs = np.linalg.solve(H_new, g)
    ew, ef = np.abs(xw[0] - xs).max(), np.abs(xf[0] - xs).max()
    floor = C * n * EPS * np.abs(xs).max()
    # a row that LEAVES makes the pivot of the small system 1 / D - j' inv(H_old) j = (1 / D) rho, rho = 1 - D j' inv(H_old) j in (0, 1]: the routine accepts
    # rho down to 1e-4 (its singularity test) and the update then carries 1 / rho times the rounding of a fresh factorisation; entering rows have rho >= 1
    Hoi = np.linalg.inv(H_old)
    amp = max([1.0] + [1.0 / (1.0 - D * j @ Hoi @ j) for j, D, enter in changes if not enter])
    assert ew <= 10 * ef * amp + floor, "%s n=%d %s: Woodbury error %.3e, fresh factorisation %.3e" % (probe.tier, n, case, ew, ef)
    if case == "4all_kinds":   # every one of the RG_WOODBURY rows matters: leaving any one out moves x far beyond the bound
        for drop in range(len(changes)):
            Hd = H_new.copy(); j, D, enter = changes[drop]
            Hd += (-D if enter else D) * np.outer(j, j)
            xd = np.linalg.solve(Hd, g)
            assert np.abs(xd - xs).max() > 10 * (10 * ef * amp + floor), "row %d of %s does not move the solution enough to be checked" % (drop, case)


@pytest.mark.parametrize("n", [24, 30])
def test_rg_woodbury_refuses_near_singular_and_leaves_x(probe, n):
    """A leaving dof row that carried almost all of the Hessian along its dof: 1 / D - j' inv(H_old) j ~ 1e-6 / D, below the 1e-4 test."""
    rng = np.random.RandomState(n)
    Hb = fam_structured(n, 5 * n, dmax=1e2)
    d = 3
    Hb[d, :] = 0.0; Hb[:, d] = 0.0; Hb[d, d] = 1e-6 * 500.0
    rows = [("dof", 0, False, 500.0)]
    _, _, tab, changes = _wood_setup(n, rows, seed=0, base=Hb)
    j, D, _ = changes[0]
    tab["sdesc"] = [d | (31 << 6)]
    H_old = as_f32(Hb + D * np.outer(np.eye(n)[d], np.eye(n)[d]))
    g = rhs(n, 4).astype(np.float32)
    _, xw, _, st, ret = probe.rg(4, H_old[None], rhs(n, 9)[None], g[None].astype(np.float64), wood=tab)
    assert ret[0] == 0, "%s: near-singular small system accepted" % probe.tier
    assert np.array_equal(xw[0].astype(np.float32).view(np.uint32), g.view(np.uint32)), "x was touched by a refused update"


# ------------------------------------------------------------------------------------------------- rb: one-wave register solves, the four-wave paths
RB_SMALL = [1, 7, 8, 9, 16, 17, 24, 25, 38, 40]
RB_MEDIUM = [41, 55, 56]
RB_LARGE = [1, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96]


def _rb_check(probe, cfg, op, n, factor):
    fams = families(n)
    As = np.stack([H for _, H in fams])
    gs = np.stack([rhs(n, i) for i in range(len(fams))])
    perm = np.random.RandomState(n).permutation(n)
    x, Ls, sc, ret = probe.rb(cfg, op, As, gs, perm)
    for b, (name, H) in enumerate(fams):
        tag = "%s rb cfg%d op%d n=%d %s" % (probe.tier, cfg, op, n, name)
        assert ret[b] == 1, tag
        check_solve(tag, H, x[b], gs[b])
        if factor:   # the factor of the scaled block S H S that the substitutions read (lower triangle)
            SHS = sc[b][:, None] * H * sc[b][None, :]
            e = np.abs(Ls[b] @ Ls[b].T - SHS).max() / np.abs(SHS).max()
            assert e <= C * n * EPS, "%s: |LL' - SHS| / |SHS| = %.3e" % (tag, e)


@pytest.mark.parametrize("n", RB_SMALL)
def test_rb_reg_solve_small(probe, n):
    _rb_check(probe, 0, 0, n, False)


@pytest.mark.parametrize("n", RB_MEDIUM)
def test_rb_reg_solve_medium(probe, n):
    _rb_check(probe, 1, 0, n, False)


@pytest.mark.parametrize("n", RB_LARGE)
@pytest.mark.parametrize("op", [0, 1], ids=["chol_mfma", "lds_chol"])
def test_rb_large_factor_and_solve(probe, op, n):
    _rb_check(probe, 2, op, n, True)


@pytest.mark.parametrize("where", [(0, 8), (0, 40), (1, 56), (2, 96), (2, 33)], ids=lambda w: "cfg%d_n%d" % w)
@pytest.mark.parametrize("kind", ["indefinite", "singular", "nan"])
def test_rb_failure_inputs_return_false(probe, where, kind):
    cfg, n = where
    H, ok_H = fam_fail(n, kind), fam_cond(n, 1e3, 3)
    for op in ([0, 1] if cfg == 2 else [0]):
        _, _, _, ret = probe.rb(cfg, op, np.stack([H, ok_H]), np.stack([rhs(n, 0), rhs(n, 1)]))
        assert ret[0] == 0 and ret[1] == 1, "%s cfg%d op%d n=%d %s: %s" % (probe.tier, cfg, op, n, kind, ret)


# ------------------------------------------------------------------------------------------------- wave primitives
def _prim(probe, seed, fx=None, K=0):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-10, 10, 64).astype(np.float32)
    v += np.repeat(np.arange(4) * 100.0, 16).astype(np.float32)   # 16-lane groups in disjoint ranges: leaks between groups show
    u = rng.uniform(-1, 1, 64).astype(np.float32)
    iv = (rng.randint(-1000, 1000, 64) + np.repeat(np.arange(4) * 5000, 16)).astype(np.int32)
    fa = rng.randn(K, 64).astype(np.float32) if K else None
    fb = rng.randn(K, 64).astype(np.float32) if K else None
    out, iout, fo = probe.prim(v, u, iv, np.arange(64, dtype=np.int32), fa, fb, fx)
    return v, u, iv, fa, fb, out, iout, fo


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_wave_reductions(probe, seed):
    v, u, iv, _, _, out, iout, _ = _prim(probe, seed)
    v64 = v.astype(np.float64)
    assert np.all(np.abs(out[:, 0] - v64.sum()) <= 6 * EPS * np.abs(v64).sum())
    assert np.all(out[:, 1] == v.max())
    assert np.all(iout[:, 0] == iv.min())
    assert np.all(out[:, 2] == v.max()) and np.all(iout[:, 1] == int(np.argmax(v)))
    for col, G in zip(range(3, 7), (2, 4, 8, 16)):
        want = v.reshape(-1, G).max(1).repeat(G)
        assert np.array_equal(out[:, col], want), "grp_max<%d>" % G
    for col, G in zip(range(2, 6), (2, 4, 8, 16)):
        assert np.array_equal(iout[:, col], iv.reshape(-1, G).min(1).repeat(G)), "grp_min_i<%d>" % G
    s16 = v64.reshape(4, 16)
    assert np.all(np.abs(out[:, 7] - s16.sum(1).repeat(16)) <= 4 * EPS * np.abs(s16).sum(1).repeat(16)), "grp_sum16"
    for src in range(64):
        assert np.all(out[:, 10 + src] == v[src]), "lane_bcast from lane %d" % src
    lane = np.arange(64)
    src = (lane & 31)
    assert np.array_equal(out[:, 8], np.where(lane < 32, v[src], u[src])), "rg_halves<0>"
    assert np.array_equal(out[:, 9], np.where(lane < 32, v[src + 32], u[src + 32])), "rg_halves<1>"


def test_wave_argmax_ties_go_to_the_smallest_index(probe):
    v = np.zeros(64, np.float32); v[[5, 17, 40, 63]] = 3.0
    out, iout, _ = probe.prim(v, v, np.zeros(64, np.int32), np.arange(64, dtype=np.int32))
    assert np.all(iout[:, 1] == 5) and np.all(out[:, 2] == 3.0)
    ix = np.arange(64, dtype=np.int32)[::-1].copy()      # the index carried by the lane decides, not the lane
    out, iout, _ = probe.prim(v, v, np.zeros(64, np.int32), ix)
    assert np.all(iout[:, 1] == 0)


def test_wave_max_below_the_dpp_fill_value(probe):
    """The device's DPP steps fill lanes without a source with -3e38 (rg_kernel.h wave_max), but the result is read from lane 63, whose
    sources are always in range: the fill never reaches it.  Contract, the same on both builds: wave_max is exact for every input, -inf and
    values below -3e38 included, and wave_argmax of an all -inf wave returns lane 0's index (not 0x7fffffff)."""
    for fill, top in ((-3e38, -2.9e38), (-3.3e38, -3.2e38), (-np.inf, -3.3e38)):
        v = np.full(64, fill, np.float32); v[9] = top
        out, iout, _ = probe.prim(v, v, np.zeros(64, np.int32), np.arange(64, dtype=np.int32))
        assert np.all(out[:, 1] == np.float32(top)) and np.all(iout[:, 1] == 9), (fill, top)
    v = np.full(64, -np.inf, np.float32)
    out, iout, _ = probe.prim(v, v, np.zeros(64, np.int32), np.arange(64, dtype=np.int32))
    assert np.all(out[:, 1] == -np.inf) and np.all(out[:, 2] == -np.inf) and np.all(iout[:, 1] == 0)


@pytest.mark.parametrize("K", [1, 2, 16])
def test_rg_mfma32_layout(probe, K):
    """acc += A B per step, A = 32 x 2 (lane l: A[l % 32][l / 32]), B = 2 x 32 (lane l: B[l / 32][l % 32]); lane l holds column l % 32,
    register r row 8 (r / 4) + 4 (l / 32) + r % 4 (rg_kernel.h)."""
    _, _, _, fa, fb, out, _, _ = _prim(probe, 10 + K, K=K)
    want = np.zeros((32, 32))
    for k in range(K):
        A = np.stack([fa[k][:32], fa[k][32:]], 1).astype(np.float64)
        B = np.stack([fb[k][:32], fb[k][32:]], 0).astype(np.float64)
        want += A @ B
    absw = np.zeros((32, 32))
    for k in range(K):
        absw += np.abs(np.stack([fa[k][:32], fa[k][32:]], 1)) @ np.abs(np.stack([fb[k][:32], fb[k][32:]], 0))
    for l in range(64):
        for r in range(16):
            row, col = 8 * (r // 4) + 4 * (l // 32) + r % 4, l % 32
            assert abs(out[l, 74 + r] - want[row, col]) <= 2 * K * EPS * absw[row, col] + 1e-30, (l, r)


def test_rcp_rsqrt_sqrt_one_ulp(probe):
    """Device: v_rcp_f32 / v_rsq_f32 / v_sqrt_f32, 1 ulp.  Emulation: 1 / x, 1 / sqrtf(x), sqrtf(x): correctly rounded except 1 / sqrtf(x), two roundings (< 2 ulp)."""
    rng = np.random.RandomState(0)
    fx = np.concatenate([np.logspace(-30, 30, 601), rng.uniform(0.5, 2.0, 200), [1e-30, 1e-15, 1.0, 4.0, 2.0 ** -126 * 4]]).astype(np.float32)
    _, _, fo = probe.prim(np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(64, np.int32), np.arange(64, dtype=np.int32), fx=fx)
    x = fx.astype(np.float64)
    for col, exact in ((0, 1.0 / x), (1, 1.0 / np.sqrt(x)), (2, np.sqrt(x))):
        ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)
        err = np.abs(fo[:, col].astype(np.float64) - exact)
        lim = 2.0 if (probe.tier == "emul" and col == 1) else 1.0
        assert np.all(err <= lim * ulp), ("rcp", "rsqrt", "sqrt")[col] + " beyond 1 ulp at %s" % fx[np.argmax(err / ulp)]
