"""The precision-sampler kernels of ccmm_ps.hip (k_ps_chol, k_ps_chol_w<W>, k_ps_prop<W>, k_ps_apply<W, forced>,
k_ps_draw1<W>, k_ps_first_store, k_ps_store) and the P | b_PS | gP records of k_elb_cond at the edges of the
band-width bucket, the 64-row LDS chunk, the censoring mask, the Philox pairing, the 256-proposal block and
the LDS residency, on the cases of tests/ps_cases.py.  Every test is one sweep; the ELB step runs last in a
sweep, so the state read back (PAI, A, sqrtht) is what the PS kernels saw, and refs.ps_draw_ld (longdouble,
dense, read off the joint density of the window) is evaluated at it.  tests/test_refs.py holds the fp64 oracle
to 1e-11 of that reference on every case.  Tolerance throughout: 1e-9 in units of max(|x|, 0.1).

Test A (every case; test E is the same on the hybrid model, where Yhatactual is the intercept of b_PS): the
missing-data draw with supplied normals, draw and centre P^-1 b against longdouble, then the unfused pair and
the first-generation factorisation bit for bit.  Test B: Philox; the host forms the same normals from
tests/philox.py (block 8, index i + n2 k, sweep 0), so ps_fill_normals (the missing-data draw) and ps_backsub's
pipelined pairs (proposal 1 of the PS branch) are each held to the generator, and the accepted index to the
first reference draw wholly below the ELB.  Test C: common random numbers engineered from the longdouble factor
(z_k = L' x_k - ybar) so that the accepted index is known: the last thread of a block, a block one thread deep,
two accepted proposals in different blocks in either order; every other proposal rejected at the last cell
substituted (chain 0) or the first (chain 1).  Test D: three data slots of unequal size in one chain set.

VARIANT TABLE (launch_ps_draw1, launch_ps_chol, launch_ps_apply; W = the bucket the case asserts)
  k_ps_draw1<16>            A, fused: w1 w2 w16_full w16_holes n1..n7 n15_w16 n16_w16 n17_w16 n64_nc64 n65_nc65 n128_w16
                            n129_w16 and the mask cases (gap_*, alternating, month0, last_month, month0_and_last);
                            B (i): n1..n7 n64_nc64 n65_nc65; E: hybrid_gaps
  k_ps_draw1<32>            A: w17_full w17_holes w32_full w32_holes
  k_ps_draw1<48>            A: w33_full w33_holes w48_full w48_holes n57_w48; B (i): n57_w48
  k_ps_draw1<64>            A: w49_holes w64_full w64_holes n63_w64 n64_w64 n65_w64 n128_w64 n129_w64, resident_last (band
                            rows in LDS) and resident_first_out (read back from ps.L)
  k_ps_chol_w<16>           A, fused=False: the cases of k_ps_draw1<16>; B (ii), C: n5 n65_nc65
  k_ps_chol_w<32>           A, fused=False: the cases of k_ps_draw1<32>; D
  k_ps_chol_w<48>           A, fused=False: the cases of k_ps_draw1<48>; B (ii), C: n57_w48
  k_ps_chol_w<64>           A, fused=False: the cases of k_ps_draw1<64>; C: n65_w64
  k_ps_chol (W <= 64)       A, option ps_chol_lds = 1: every case of bucket 16, 32, 48, 64
  k_ps_chol (W = 80)        A: w65_full w68_full, 128 threads, the only factorisation there (kernel_times shows that
                            the pair ran); test_ps_w80_proposals
  k_ps_apply<W, true>       A, fused=False and ps_chol_lds = 1, W = 16 | 32 | 48 | 64: the cases above per bucket;
                            W = 80: w65_full w68_full
  k_ps_prop<16>, k_ps_apply<16, false>   B (ii)-(iv): n1..n7 n64_nc64 n65_nc65; C: n5 n65_nc65
  k_ps_prop<32>, k_ps_apply<32, false>   D (the wide slot sets the bucket; the n = 3 slot runs in it)
  k_ps_prop<48>, k_ps_apply<48, false>   B: n57_w48; C: n57_w48
  k_ps_prop<64>, k_ps_apply<64, false>   C: n65_w64
  k_ps_prop<80>, k_ps_apply<80, false>   test_ps_w80_proposals: w65_full
  k_ps_first_store, k_ps_store           every test (NaN beyond the shorter windows: D)

MEASURED on an MI355X, worst over cases and chains, in the units of the assertions (bound 1e-9):
  A  draw 1.0e-12 (resident_first_out, 244 cells), centre 4.0e-13 (resident_last); every case of fewer than
     100 cells below 1e-13
  B  draw and proposal 1 5.3e-14, centre 1.6e-14 (n57_w48); accepted proposals' shadow rates 1.1e-14.  Reference
     and device ndxAccept: n1 19 | 9, n2 147 | 97, n3 26 | 49, n5 190 | 152, n65_nc65 74 | 0, none in n4, n6, n7,
     n64_nc64, n57_w48; closest cell to the ELB over all proposals read 4.0e-6 (n64_nc64): no chain left out
  E  draw 3.1e-15, centre 1.6e-15
  C, D  shadow rates and proposal 1 below 1e-14"""
import numpy as np
import pytest

import philox
import ps_cases as pc

pytestmark = pytest.mark.gpu

TOL = 1e-9
STATE = ("PAI", "A", "sqrtht", "h", "sqrtPHI")
RNG_PS = 8  # CCMM_RNG_PS


def _chains(pkg, ctx, c, su, B, *, crn, cap=1, seed=20240611, ndata=1, T=None, elbTmax=None):
    lin = su.lin
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T if T is None else T, B=B, ndata=ndata, crn=crn,
                    model=pkg.MODEL_HYBRID if c.hybrid else pkg.MODEL_BLOCKHYBRID, Ns=c.Ns,
                    elbTmax=su.elbT if elbTmax is None else elbTmax, elb_gibbsburn=su.gibbsburn, elb=pc.ELB,
                    store_capacity=cap, seed=seed)
    if ndata == 1:
        ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
        ch.set_elb_model(su.ndxS, None if c.hybrid else su.actualrateBlock)
        ch.set_elb_slot(0, su.elbT0, su.sNaN)
    return ch


def _set_state(ch, sts):
    ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in STATE])


def _record(ch, seed, z):
    """A CRN record of one sweep: every block random (the same numbers whatever the PS block's length, which comes
    last), the PS block the supplied normals z[c] (n_c x NP, column-major: cell i of proposal k at i + n k)."""
    crn = ch.draw_crn(np.random.default_rng(seed), 1)
    off, length, _ = ch.crn_layout()["PS"]
    crn[off:off + length] = 0.0
    for c, zc in enumerate(z):
        flat = np.asarray(zc, float).ravel(order="F")
        assert flat.size <= length
        crn[off:off + flat.size, 0, c] = flat
    return crn


def _cv(a, m):
    """The cells of the mask m (Ns x elbT) of a in the order of the reference: month-major, rates in index order."""
    return a.T[m.T]


def _window(su):
    lin = su.lin
    return lin.data[lin.p + su.elbT0:lin.p + lin.T, :][:, su.ndxS].T


def _missing_run(pkg, ctx, c, su, sts, z, fused=True, lds=0, crn=True, seed=20240611):
    ch = _chains(pkg, ctx, c, su, len(sts), crn=crn, seed=seed)
    ch.set_option("ps_chol_lds", lds)
    ch.set_elb_treatment(missing=True, fused=fused)
    _set_state(ch, sts)
    ch.profile(True)
    ch.sweep(1, crn=_record(ch, 5, z) if crn else None, store=True)
    out = dict(miss=ch.get_missingrate()[0], mean=ch.get_ps_mean(), state=ch.get_state(), status=ch.get_status(),
               S=ch.get_shadowrate(), kt=ch.kernel_times())
    ch.close()
    return out


def _check_draw(name, c, su, out, z, what):
    """Test A's assertion: the draw and the centre against longdouble, the other cells the window's data bit for
    bit, the centre NaN off the mask, status clean.  Returns the two errors."""
    worst = [0.0, 0.0]
    m = su.sNaN
    assert np.all(out["status"] == 0), out["status"]
    for ch_ in range(out["miss"].shape[-1]):
        st = out["state"]
        mean, _, _, draws = pc.draw_reference(c, su, st["PAI"][..., ch_], st["A"][..., ch_],
                                              st["sqrtht"][:su.lin.T, :, ch_], z[ch_][:, :1])
        got, ctr = out["miss"][:, :su.elbT, ch_], out["mean"][:, :su.elbT, ch_]
        e = pc.rel_err(_cv(got, m), draws[:, 0]), pc.rel_err(_cv(ctr, m), mean)
        print(f"{name} {what} chain {ch_}: n {c.n} wmax {c.wmax} bucket {c.bucket}: draw {e[0]:.2e} centre {e[1]:.2e}")
        assert e[0] < TOL and e[1] < TOL, (name, what, ch_, e)
        np.testing.assert_array_equal(got[~m], _window(su)[~m])
        assert np.all(np.isnan(ctr[~m])) and np.all(np.isfinite(ctr[m]))
        worst = [max(a, b) for a, b in zip(worst, e)]
    return worst


def _factor_and_draw(pkg, ctx, name):
    c, su = pc.build(name)
    sts = pc.start_states(su)
    rng = np.random.default_rng([11, c.n, c.p])
    z = [rng.standard_normal((c.n, 1)) for _ in sts]
    fused = _missing_run(pkg, ctx, c, su, sts, z)
    _check_draw(name, c, su, fused, z, "fused")
    assert not np.array_equal(fused["miss"][..., 0], fused["miss"][..., 1])
    if c.bucket > 64:  # the unfused pair with k_ps_chol is the only form
        assert fused["kt"]["k_ps_chol"][1] > 0 and fused["kt"]["k_ps_prop"][1] > 0, fused["kt"]
        return
    assert fused["kt"]["k_ps_chol"][1] > 0 and fused["kt"]["k_ps_prop"][1] == 0, fused["kt"]  # k_ps_draw1 alone
    for kw in (dict(fused=False), dict(lds=1)):
        o = _missing_run(pkg, ctx, c, su, sts, z, **kw)
        assert o["kt"]["k_ps_chol"][1] > 0 and o["kt"]["k_ps_prop"][1] > 0, o["kt"]
        assert np.all(o["status"] == 0)
        np.testing.assert_array_equal(o["miss"], fused["miss"], err_msg=f"{name} {kw}")
        np.testing.assert_array_equal(o["mean"], fused["mean"], err_msg=f"{name} {kw}")
        np.testing.assert_array_equal(o["state"]["PAI"], fused["state"]["PAI"])


# ---------------------------------------------------------------- A: factor and draw, CRN, every case
@pytest.mark.parametrize("name", pc.BAND + pc.COUNT + pc.MASK + pc.RESIDENCY)
def test_factor_and_draw_against_longdouble(pkg, ctx, name):
    _factor_and_draw(pkg, ctx, name)


# ---------------------------------------------------------------- E: the hybrid model's b_PS off the contiguous window
@pytest.mark.parametrize("name", pc.HYBRID)
def test_hybrid_factor_and_draw_against_longdouble(pkg, ctx, name):
    assert pc.case(name).hybrid
    _factor_and_draw(pkg, ctx, name)


# ---------------------------------------------------------------- B: Philox numbering
_LEFT_OUT = []
NP_PHILOX = 600


def _first_accepted(draws, upto=None):
    """(first k with every cell below the ELB or None, smallest |x - ELB| over the proposals up to and including it)."""
    ok = np.all(draws < pc.LD(pc.ELB), axis=0)
    k = int(np.argmax(ok)) if ok.any() else None
    seen = draws if k is None else draws[:, :k + 1]
    return k, float(np.min(np.abs(seen - pc.LD(pc.ELB))))


@pytest.mark.parametrize("name", pc.PHILOX)
def test_philox_numbering_and_acceptance(pkg, ctx, name):
    c, su = pc.build(name)
    sts, n, NP, seed = pc.start_states(su), c.n, NP_PHILOX, 777001
    n2 = n + (n & 1)
    idx = np.arange(n)[:, None] + n2 * np.arange(NP)[None, :]
    z = [philox.normal(seed, ch_, 0, RNG_PS, idx) for ch_ in range(len(sts))]
    one = _missing_run(pkg, ctx, c, su, sts, z, crn=False, seed=seed)                 # (i) ps_fill_normals
    _check_draw(name, c, su, one, z, "philox draw")
    ch = _chains(pkg, ctx, c, su, len(sts), crn=False, seed=seed)                     # (ii) ps_backsub's pairs
    ch.set_elb_ps(NP, 1)
    ch.keep_missingrate(True)
    _set_state(ch, sts)
    ch.sweep(1, store=True)
    out = dict(miss=ch.get_missingrate()[0], mean=ch.get_ps_mean(), state=ch.get_state(), status=ch.get_status())
    S, ps = ch.get_shadowrate(), ch.get_ps()
    ch.close()
    np.testing.assert_array_equal(out["state"]["PAI"], one["state"]["PAI"])
    _check_draw(name, c, su, out, z, "philox proposal 1")
    np.testing.assert_array_equal(out["miss"], one["miss"])
    np.testing.assert_array_equal(out["mean"], one["mean"])
    m = su.sNaN
    for ch_ in range(len(sts)):
        st = out["state"]
        _, _, _, draws = pc.draw_reference(c, su, st["PAI"][..., ch_], st["A"][..., ch_], st["sqrtht"][:su.lin.T, :, ch_],
                                           z[ch_])
        k, gap = _first_accepted(draws)
        got = int(ps["stackAccept"][0, ch_])
        print(f"{name} chain {ch_}: reference ndxAccept {0 if k is None else k + 1}, device {got}, closest cell {gap:.1e}")
        if gap < 1e-6:                                                                # (iii) a decision within rounding
            _LEFT_OUT.append((name, ch_))
            continue
        assert got == (0 if k is None else k + 1), (name, ch_, got, k)
        assert int(ps["countAccept"][ch_]) == (k is not None) and int(ps["countAcceptBurnin"][ch_]) == 0
        if k is None:
            assert np.all(S[:, :su.elbT, ch_][m] <= pc.ELB)                          # the Gibbs draw
        else:                                                                         # (iv) k_ps_apply at kmin = k
            e = pc.rel_err(_cv(S[:, :su.elbT, ch_], m), draws[:, k])
            print(f"{name} chain {ch_}: accepted proposal {k + 1}, shadow rates {e:.2e}")
            assert e < TOL, (name, ch_, k, e)
        np.testing.assert_array_equal(S[:, :su.elbT, ch_][~m], _window(su)[~m])
    assert len(_LEFT_OUT) * 10 <= 2 * len(pc.PHILOX), _LEFT_OUT                      # one chain in ten at most


# ---------------------------------------------------------------- C: engineered acceptance, CRN
_PASS1 = {}
CONFIGS = pc.CONFIGS


def _ps_run(pkg, ctx, c, su, sts, NP, z, store=True):
    ch = _chains(pkg, ctx, c, su, len(sts), crn=True)
    ch.set_elb_ps(NP, 1)
    ch.keep_missingrate(True)
    _set_state(ch, sts)
    ch.sweep(1, crn=_record(ch, 5, z), store=store)
    out = dict(state=ch.get_state(), status=ch.get_status(), S=ch.get_shadowrate(), ps=ch.get_ps(), mean=ch.get_ps_mean())
    if store:
        out["miss"] = ch.get_missingrate()[0]
    ch.close()
    return out


def _pass1(pkg, ctx, name):
    """The sweep with z = 0: the state the PS kernels see (the PS normals do not influence it) and its longdouble
    factor and ybar per chain."""
    if name not in _PASS1:
        c, su = pc.build(name)
        sts = pc.start_states(su)
        o = _ps_run(pkg, ctx, c, su, sts, 1, [np.zeros((c.n, 1)) for _ in sts])
        st = o["state"]
        ref = [pc.draw_reference(c, su, st["PAI"][..., k], st["A"][..., k], st["sqrtht"][:su.lin.T, :, k],
                                 np.zeros((c.n, 1))) for k in range(len(sts))]
        _PASS1[name] = (sts, st, ref)
    return _PASS1[name]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", pc.ENGINEERED)
def test_engineered_acceptance(pkg, ctx, name, config):
    c, su = pc.build(name)
    NP, accepted, want, store = CONFIGS[config]
    sts, st1, ref = _pass1(pkg, ctx, name)
    # every other proposal: chain 0 rejected at cell 0 (the last one substituted), chain 1 at the top cell
    x = [pc.targets(c.n, NP, accepted, early=bool(k)) for k in range(len(sts))]
    z = [pc.engineered_normals(ref[k][2], ref[k][1], x[k]) for k in range(len(sts))]
    o = _ps_run(pkg, ctx, c, su, sts, NP, z, store=store)
    np.testing.assert_array_equal(o["state"]["PAI"], st1["PAI"])   # the same state as in pass 1
    np.testing.assert_array_equal(o["state"]["sqrtht"], st1["sqrtht"])
    assert np.all(o["status"] == 0)
    m = su.sNaN
    for k in range(len(sts)):
        draws = refs_draws(ref[k], z[k])
        assert float(np.min(np.abs(draws - pc.LD(pc.ELB)))) >= 0.5
        assert _first_accepted(draws)[0] == (want - 1 if want else None)
        S = o["S"][:, :su.elbT, k]
        if store:
            assert int(o["ps"]["stackAccept"][0, k]) == want, (name, config, k, o["ps"]["stackAccept"])
            e1 = pc.rel_err(_cv(o["miss"][:, :su.elbT, k], m), draws[:, 0])       # proposal 1, accepted or not
            assert e1 < TOL, (name, config, k, e1)
            np.testing.assert_array_equal(o["miss"][:, :su.elbT, k][~m], _window(su)[~m])
        assert int(o["ps"]["countAccept"][k]) == (1 if want and store else 0)
        assert int(o["ps"]["countAcceptBurnin"][k]) == (1 if want and not store else 0)
        if want:
            e = pc.rel_err(_cv(S, m), draws[:, want - 1])
            print(f"{name} {config} chain {k}: accepted {want}, shadow rates {e:.2e}")
            assert e < TOL, (name, config, k, e)
        else:
            assert np.all(S[m] <= pc.ELB) and not np.any(np.abs(S[m] - (pc.ELB - 1.0)) < 1e-6)  # the Gibbs draw
        np.testing.assert_array_equal(S[~m], _window(su)[~m])


def refs_draws(ref, z):
    """The longdouble draws L'^-1 (ybar + z_k) of one chain from its factor (ref = (mean, ybar, L, .))."""
    return pc.refs.bwd_cols_ld(ref[2], ref[1][:, None] + np.asarray(z).astype(pc.LD))


def test_ps_w80_proposals(pkg, ctx):
    """k_ps_prop<80> and k_ps_apply<80, false> behind k_ps_chol on 128 threads: proposal 3 of 4 engineered to be
    the only one accepted."""
    name = "w65_full"
    c, su = pc.build(name)
    assert c.bucket == 80
    sts, st1, ref = _pass1(pkg, ctx, name)
    x = [pc.targets(c.n, 4, [2], early=bool(k)) for k in range(len(sts))]
    z = [pc.engineered_normals(ref[k][2], ref[k][1], x[k]) for k in range(len(sts))]
    o = _ps_run(pkg, ctx, c, su, sts, 4, z)
    np.testing.assert_array_equal(o["state"]["PAI"], st1["PAI"])
    assert np.all(o["status"] == 0)
    for k in range(len(sts)):
        draws = refs_draws(ref[k], z[k])
        assert int(o["ps"]["stackAccept"][0, k]) == 3
        e = pc.rel_err(_cv(o["S"][:, :su.elbT, k], su.sNaN), draws[:, 2]), pc.rel_err(_cv(o["miss"][:, :su.elbT, k], su.sNaN), draws[:, 0])
        print(f"{name} chain {k}: shadow rates {e[0]:.2e}, proposal 1 {e[1]:.2e}")
        assert max(e) < TOL, e


# ---------------------------------------------------------------- D: slots of unequal size
def test_slots_wide_small_and_empty(pkg, ctx):
    """One chain set over three data slots: a wide one (wmax 17: the set's bucket is 32), one with n = 3 cells
    (n < nmax, a band narrower than the bucket, a shorter window) and one whose window holds no censored cell."""
    from test_gpu_vintages import _stack_state
    Ns, p = 3, 5
    masks = [pc.periodic(3, 16, 1, 15, 6, (2,)), pc.cells(3, 9, [(0, 2), (2, 2), (1, 3)]), np.zeros((3, 6), bool)]
    assert [pc.band(m, p) for m in masks] == [(17, 32, 40, 14), (3, 16, 3, 2), (1, 16, 0, 0)]
    sus = [pc.make_setup(Ns, p, m, seed=50 + k, T=T) for k, (m, T) in enumerate(zip(masks, (64, 60, 58)))]
    c = pc.Case("slots", Ns, p, 1, None, 17, 32, 40, 14, True, False)
    slots = [0, 1, 2, 2, 1, 0]
    B, NP, Tmax, ETmax = len(slots), 8, 64, 16
    sts = [pc.start_states(sus[s], B=1, seed=300 + k)[0] for k, s in enumerate(slots)]
    ch = _chains(pkg, ctx, c, sus[0], B, crn=True, ndata=3, T=Tmax, elbTmax=ETmax)
    for k, su in enumerate(sus):
        L = su.lin
        ch.set_data(k, L.Y, L.X, L.iVdiag, L.iVb, L.sPHI, L.Vol_0mean, L.Vol_0vcvsqrt)
    ch.set_slots(slots)
    ch.set_elb_model(sus[0].ndxS, sus[0].actualrateBlock)
    for k, su in enumerate(sus):
        ch.set_elb_slot(k, su.elbT0, su.sNaN)
    ch.set_elb_ps(NP, 1)
    ch.keep_missingrate(True)
    ch.set_state(*_stack_state(sts, Tmax))
    rng = np.random.default_rng(61)
    z = [rng.standard_normal((int(sus[s].sNaN.sum()), NP)) for s in slots]
    ch.sweep(1, crn=_record(ch, 6, z), store=True)
    st, S, miss, mean, ps = ch.get_state(), ch.get_shadowrate(), ch.get_missingrate()[0], ch.get_ps_mean(), ch.get_ps()
    assert np.all(ch.get_status() == 0)
    ch.close()
    for k, s in enumerate(slots):
        su, m = sus[s], sus[s].sNaN
        assert np.all(np.isnan(miss[:, su.elbT:, k]))                                  # beyond the slot's own window
        np.testing.assert_array_equal(S[:, :su.elbT, k][~m], _window(su)[~m])
        if s == 2:
            assert int(ps["stackAccept"][0, k]) == 0 and not m.any() and np.all(np.isnan(mean[:, :, k]))
            continue
        cs = c._replace(n=int(m.sum()))
        ctr, _, _, draws = pc.draw_reference(cs, su, st["PAI"][..., k], st["A"][..., k], st["sqrtht"][:su.lin.T, :, k], z[k])
        e = pc.rel_err(_cv(miss[:, :su.elbT, k], m), draws[:, 0]), pc.rel_err(_cv(mean[:, :su.elbT, k], m), ctr)
        print(f"slot {s} chain {k}: n {cs.n}: proposal 1 {e[0]:.2e} centre {e[1]:.2e}")
        assert max(e) < TOL, (k, e)
        np.testing.assert_array_equal(miss[:, :su.elbT, k][~m], _window(su)[~m])
        assert np.all(np.isnan(mean[:, :su.elbT, k][~m])) and np.all(np.isnan(mean[:, su.elbT:, k]))
        acc, gap = _first_accepted(draws)
        if gap >= 1e-6:
            assert int(ps["stackAccept"][0, k]) == (0 if acc is None else acc + 1)
            if acc is not None:
                assert pc.rel_err(_cv(S[:, :su.elbT, k], m), draws[:, acc]) < TOL
