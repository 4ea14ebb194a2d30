"""The library's own launch arithmetic, on the CPU: tests/launch_plans_main.cpp includes the kernel units'
headers (ccmm_elb.h, ccmm_sweep.h, ccmm_fcst.h, ccmm_lag.h), calls no HIP runtime function and prints the plans
and LDS layouts the host launchers use.  Checked against the restatements of tests/elb_cases.py on every ELB
edge case, so that the edge asserts there (n65_lagbatch -> kb 10, long_w4 -> 4, long_w1 -> 1) are statements
about the library, and against the layout comments of the kernels region by region.  The predictive-density
launch (fcst_reg_path, fcst_chunk, fcst_variant, fcst_paths_lds_doubles) is checked on every case of
tests/fcst_cases.py in the same way, and the GIRF launch (ccmm_girf.h girf_plan, girf_lds, girf_fast_lds) on every
case of tests/girf_cases.py.  The large-N path (ccmm_bign.h: the padded Gram dimension, the LDS sizes and the SV
scratch for every N = 33..128; ccmm_big.h: big_solve_plan) is checked against tests/bign_cases.py, and phi_plan
(ccmm_sweep.h) with every value of option phi_stage against tests/phi_cases.py.  The same program
prints the library's Philox4x32-10 words (Rng::raw), which pin tests/philox.py bit for bit."""
import subprocess

import pytest

import bign_cases as BC
import elb_cases as EC
import fcst_cases as FC
import girf_cases as GC
import phi_cases as PC
import philox
from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
LDS_CU = 160 * 1024
WANTS = (1, 4, 8)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """query(lines) -> one list of output tokens per line, from one run of the compiled program."""
    exe = tmp_path_factory.mktemp("launch_plans") / "launch_plans"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "launch_plans_main.cpp"), "-o", str(exe)],
                   check=True)

    def query(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        rows = [r.split() for r in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return query


def _layout(row):
    """(total bytes, [(region, offset)] in layout order) of a layout line."""
    return int(row[0]), [(t.split(":")[0], int(t.split(":")[1])) for t in row[1:]]


def _check_layout(row, sizes, doubles):
    """The regions start at 0, follow each other without gap or overlap in the order and with the sizes the
    kernel's layout comment gives, end at the size the launcher asks for, and the double regions are 8-byte
    aligned."""
    total, regions = _layout(row)
    assert [r for r, _ in regions] == [r for r, _ in sizes]
    off = 0
    for (name, got), (_, size) in zip(regions, sizes):
        assert got == off, (name, got, off)
        assert name not in doubles or got % 8 == 0, name
        off += size
    assert total == off


def test_cond_plan_and_gibbs_waves_match_the_restatement(plans):
    names = list(EC.CASES)
    cases = [EC.CASES[n] for n in names]
    cond = plans([f"cond {c.Ny} {c.p} {c.Ns}" for c in cases])
    for c, row in zip(cases, cond):
        assert tuple(map(int, row[:3])) == EC.cond_launch(c.Ny, c.p, c.Ns), c.name
        assert int(row[3]) <= 96 * 1024 + c.Ny * c.Ny * 8 and int(row[3]) <= LDS_CU, c.name
    waves = plans([f"waves {c.T} {c.Ns} {w}" for c in cases for w in WANTS])
    got = {(c.name, w): int(r[0]) for (c, w), r in zip(((c, w) for c in cases for w in WANTS), waves)}
    for c in cases:
        for w in WANTS:
            assert got[c.name, w] == EC.gibbs_waves(c.T, c.Ns, w), (c.name, w)
    # the edges the cases were built for
    assert tuple(map(int, cond[names.index("n65_lagbatch")][:3])) == (256, 0, 10)
    assert [got["long_w4", w] for w in WANTS] == [1, 4, 4]
    assert [got["long_w1", w] for w in WANTS] == [1, 1, 1]


def test_wave_kernel_lds_layouts(plans):
    cases = list(EC.CASES.values())
    waves = plans([f"waves {c.T} {c.Ns} {w}" for c in cases for w in WANTS])
    q, want = [], []
    for (c, w), r in zip(((c, w) for c in cases for w in WANTS), waves):
        W, pg, it = int(r[0]), c.T * c.Ns * 8, c.T * 4
        if W > 1:  # k_elb_gibbs_wf: Sl | Ul[W] | Zl[W] | Tm | reach | prog[2][W] | one spare int
            q.append(f"wf {c.T} {c.Ns} {W}")
            want.append([("Sl", pg), ("Ul", W * pg), ("Zl", W * pg), ("Tm", it), ("reach", it), ("prog", 2 * W * 4),
                         ("spare", 4)])
        if W == 8:  # k_elb_gibbs_mp<NS, WPC, 8 / WPC>: the same with WPC waves and prog[WPC + 1]
            for wpc in (4, 2):
                q.append(f"mp {c.T} {c.Ns} {wpc}")
                want.append([("Sl", pg), ("Ul", wpc * pg), ("Zl", wpc * pg), ("Tm", it), ("reach", it),
                             ("prog", (wpc + 1) * 4), ("spare", 4)])
    assert any(x.startswith("wf") and x.endswith(" 4") for x in q) and any(x.startswith("mp") for x in q)
    for line, row, sizes in zip(q, plans(q), want):
        _check_layout(row, sizes, {"Sl", "Ul", "Zl"})
        assert int(row[0]) <= LDS_CU, line  # every W elb_gibbs_waves returns fits one CU's LDS


def test_octet_and_draw1_lds_layouts(plans):
    cases = list(EC.CASES.values())
    q = [f"oct {c.T} {c.Ns}" for c in cases]
    for c, row in zip(cases, plans(q)):
        _check_layout(row, [("Sl", c.T * c.Ns * 8), ("Tm", c.T * 4), ("reach", c.T * 4)], {"Sl"})
    # k_ps_draw1<W>: k_ps_chol_w's doubles, L^-1 b, the normals, the resident band rows, then the int lists;
    # nmax = the case's censored cells (odd counts included: the ints follow the doubles)
    q, want = [], []
    for c in cases:
        nmax = int(EC.mask_of(c).sum())
        for W in (16, 32, 48, 64):
            for res in (0, 1):
                q.append(f"draw1 {W} {c.T} {nmax} {res}")
                want.append([("prow", 64 * W * 8), ("pb", 64 * 8), ("sL", W * 8), ("ybl", nmax * 8), ("zl", nmax * 8),
                             ("Ll", res * nmax * W * 8), ("scens", c.T * 4), ("info", nmax * 4), ("cellL", nmax * 4)])
    for row, sizes in zip(plans(q), want):
        _check_layout(row, sizes, {"prow", "pb", "sL", "ybl", "zl", "Ll"})


def test_prep_and_sweep_plans(plans):
    # k_elb_prep: X0 | Phi | Yb - yhat | Yb while they fit; the row split below 128 chains
    def prep(N, p, T, B):
        lds, phi = (2 + N * p + N * (N * p + 1)) * 8, 1
        if lds > LDS_CU:
            lds, phi = (2 + N * p) * 8, 0
        if phi and lds + 2 * T * N * 8 <= LDS_CU:
            lds, phi = lds + 2 * T * N * 8, 3
        rows, wg = 0, 1
        if phi & 2 and B < 128:
            per = max(1, 256 // B)
            rows = max(16, -(-T // per))
            wg = -(-T // rows)
        return [lds, phi, rows, wg]
    shapes = [(c.Ny, c.p, c.T, c.B) for c in EC.CASES.values()] + [(20, 12, 165, 256), (20, 12, 165, 1), (120, 12, 165, 4)]
    for s, row in zip(shapes, plans(["prep %d %d %d %d" % s for s in shapes])):
        assert list(map(int, row)) == prep(*s), s
    assert prep(20, 12, 165, 256)[1] == 3 and prep(120, 12, 165, 4)[1] == 0 and prep(20, 12, 165, 1)[3] > 1
    # the per-chain kernels' bucket and the staging decisions of the A-step and PHI (N = 20, T = 750: E staged,
    # 138 KB in all; N = 32 at TP = 768: neither E nor eta fits beside the rest)
    rows = plans(["misc 20 241 256 768 22", "misc 32 385 448 768 34", "misc 8 17 64 96 10", "misc 9 19 64 96 11"])
    r20, r32, r8, r9 = ([int(x) for x in r] for r in rows)
    assert (r20[0], r32[0], r8[0], r9[0]) == (20, 32, 8, 20)
    tot = 19 * 20 * 21 // 6 + 20 * 19 // 2 + 8
    assert r20[1:3] == [(tot + 400 + 20 * 768) * 8, tot + 400] and 138_000 < r20[1] <= LDS_CU
    assert r20[3:5] == [(4 * 20 * 21 + 20 * 790) * 8, 3]
    assert r32[2] == -1 and r32[4] == 0 and r32[3] == 4 * 32 * 33 * 8
    assert all(r[1] <= LDS_CU and r[3] <= LDS_CU and r[5:7] == [1, 1] for r in (r20, r32, r8, r9))
    assert (r8[7], r32[7]) == (1, 0)  # the lag solve's resident design: N = 8 at TP = 96 fits, N = 32 at 768 does not


def test_phi_plans_match_the_restatement(plans):
    """phi_plan (ccmm_sweep.h) on every case of tests/phi_cases.py: the bytes and stage bits of the default launch
    through the `misc` query, and those of every value of option phi_stage; the case list holds all three plans, the
    byte boundaries sit where the cases put them, and every staging-round case lands on its round count."""
    cases = list(PC.CASES) + [PC.MULTI[:3]]
    for (N, T, dPHI), row in zip(cases, plans([f"misc {N} {N + 1} 64 {PC.round_up(T, 32)} {dPHI}" for N, T, dPHI in cases])):
        lds, bits = int(row[3]), int(row[4])
        assert (lds, bits) == PC.plan(N, T, dPHI), (N, T, dPHI)
        assert bits == PC.CASES.get((N, T, dPHI), 3) and lds <= LDS_CU, (N, T, dPHI)
    q = [(c, m) for c in cases for m in (0, 1, 2, 3)]
    for ((N, T, dPHI), m), row in zip(q, plans([f"phi {N} {PC.round_up(T, 32)} {dPHI} {m}" for (N, T, dPHI), m in q])):
        assert (int(row[0]), int(row[1])) == PC.plan(N, T, dPHI, m), (N, T, dPHI, m)
        want = PC.plan(N, T, dPHI)[1] & m
        assert int(row[1]) == (want if want & 1 else 0), (N, T, dPHI, m)   # Z is never staged without eta
    assert set(PC.CASES.values()) == {0, 1, 3}
    # to the byte: 160 KiB stages eta and Z, one double per row more does not; then eta alone to its own limit
    assert PC.plan(32, 97, 380)[0] == PC.plan(5, 4064, 8)[0] == LDS_CU
    assert PC.plan_bytes(32, 97, 381)[2] == LDS_CU + 32 * 8 and PC.plan_bytes(5, 4064, 9)[2] == LDS_CU + 5 * 8
    assert PC.plan_bytes(32, 480, 35)[1] <= LDS_CU < PC.plan_bytes(32, 481, 35)[1]
    assert PC.plan_bytes(5, 4064, 9)[1] <= LDS_CU < PC.plan_bytes(5, 4065, 8)[1]
    assert PC.plan(20, 750, 23) == (140_000, 3)
    # staging rounds of 4096 doubles
    for (N, T, dPHI), (which, n, r) in PC.ROUNDS.items():
        assert n == (N * PC.round_up(T, 32) if which == "eta" else N * (T + dPHI)), (N, T, dPHI)
        assert PC.rounds(N, T, dPHI)[which == "z"] == r == -(-n // 4096), (N, T, dPHI)
    assert {(w, n % 4096 == 0) for w, n, _ in PC.ROUNDS.values()} == {("eta", True), ("eta", False), ("z", True), ("z", False)}


def test_fcst_plans_match_the_restatement(plans):
    """Every shape case of tests/fcst_cases.py: fcst_reg_path, fcst_chunk in both forms, the k_fcst<RN> instance
    and the chunk and LDS bytes launch_fcst takes, with option fcst_reg on and off; then the variant table of
    tests/test_gpu_fcst_edges.py's docstring, as statements about the library."""
    cases = list(FC.CASES.values())
    q = [(c, opt) for c in cases for opt in (1, 0)]
    got = {}
    for (c, opt), row in zip(q, plans([f"fcst {c.N} {c.p} {c.H} 0 {opt}" for c, opt in q])):
        r = list(map(int, row))
        Kx = c.N * c.p + 1
        reg = FC.reg_path(c.N, c.p) and bool(opt)
        hc = FC.chunk(c.N, Kx, c.p, c.H, reg)
        assert r == [int(FC.reg_path(c.N, c.p)), FC.chunk(c.N, Kx, c.p, c.H, True), FC.chunk(c.N, Kx, c.p, c.H, False),
                     FC.variant(c.N, c.p, 0, bool(opt)), hc, FC.paths_lds_doubles(c.N, Kx, c.p, hc, reg) * 8], (c.name, opt)
        assert r[5] <= LDS_CU, c.name
        got[c.name, opt] = (r[3], r[4])
    rn = {n: got[n, 1][0] for n in FC.CASES}
    assert [n for n in rn if rn[n] == 20] == ["n2_p2", "n16_p3", "n20_p4_h17", "h15", "h33", "nd1"]
    assert [n for n in rn if rn[n] == 21] == ["n3_p1", "n19_p5", "n21_p12_h16", "h1"]
    assert [n for n in rn if rn[n] == 0] == ["n22_p2", "n31_p3", "n32_p1", "n8_p13", "n21_p13", "n32_p15_h25"]
    assert all(got[n, 0][0] == 0 for n in FC.CASES)  # fcst_reg = 0: always PAI in LDS
    assert got["n32_p15_h25", 1] == (0, 13) and FC.chunks(32, 15, 25) == [13, 12]  # 25 does not fit, 13 does
    assert FC.chunks(20, 4, 17) == [16, 1] and FC.chunks(4, 2, 33) == [16, 16, 1] and FC.chunks(21, 12, 16) == [16]
    assert FC.chunks(6, 3, 15) == [15] and FC.chunks(5, 2, 1) == [1]
    assert FC.chunks(20, 4, 17, reg_opt=False) == [17]  # the LDS form takes the horizons whole
    # the hybrid model never takes the register path; the refused shape does not fit at one horizon per chunk
    assert plans(["fcst 8 2 5 2 1"])[0][:1] == ["0"] and plans(["fcst 8 2 5 2 1"])[0][3] == "0"
    r = list(map(int, plans(["fcst 32 19 1 0 1"])[0]))
    assert r[4] == 1 and r[5] > LDS_CU
    # no register-path shape is refused by the drop-in's LDS check (made with the LDS form): the largest fits
    assert FC.paths_lds_doubles(21, 253, 12, 1) * 8 <= LDS_CU


def test_girf_plans_match_the_case_table(plans):
    """Every case of tests/girf_cases.py takes the kernel its table entry names (the table of
    tests/test_gpu_girf_edges.py's docstring), with the nks, thread count and LDS bytes of the restatement; the two
    LDS layouts follow the kernels' comments region by region; the bucket limits sit where the cases put them."""
    cases = list(GC.CASES.values())
    kern = lambda r: f"fast{r[0]}" if r[0] >= 0 else f"g{r[1]}"
    rows = [list(map(int, r)) for r in plans([f"girf {c.N} {c.p} {c.Ny} {int(c.generic)}" for c in cases])]
    for c, r in zip(cases, rows):
        assert kern(r) == c.kernel, (c.name, r)
        assert (kern(r), r[2], r[3], r[4]) == GC.plan(c.N, c.p, c.Ny, c.generic), (c.name, r)
        assert r[3] == 64 * -(-c.N // 16) <= 128 and r[4] <= LDS_CU, c.name  # one wave per 16 equations, launch bound 128
    got = {c.name: (kern(r), r[2]) for c, r in zip(cases, rows)}
    assert {k for k, _ in got.values()} == {"g32", "g64", "g96", "fast0", "fast4", "fast8"}
    assert [got[n] for n in ("n7_p15_bh1", "n8_p15", "n5_p21_bh1", "n15_p16", "n16_p15", "n12_p19_bh1", "n32_p9_bh7",
                             "n20_p12_bh10")] == \
        [("g32", 32), ("g64", 33), ("g64", 33), ("g64", 64), ("g96", 65), ("g96", 65), ("g96", 96), ("g96", 96)]
    assert got["n20_p12_bh6_generic"] == ("g96", 84) and got["n20_p12_bh6"] == ("fast8", 84)
    big = next(r for c, r in zip(cases, rows) if c.name == "n32_p9_bh7")
    assert big[4] > 64 * 1024  # over the default dynamic-LDS limit: the launcher has to raise it
    # layouts
    gen = [(c, r) for c, r in zip(cases, rows) if r[0] < 0]
    for (c, r), row in zip(gen, plans([f"girfg {c.N} {c.p} {r[2]}" for c, r in gen])):
        _check_layout(row, GC.generic_regions(c.N, c.p, r[2]), {"X", "logsv", "ybuf", "nrm"})
        assert int(row[0]) == r[4], c.name
    fast = [(c, r) for c, r in zip(cases, rows) if r[0] >= 0]
    for (c, r), row in zip(fast, plans([f"girff {c.N} {r[0]}" for c, r in fast])):
        _check_layout(row, GC.fast_regions(c.N, r[0]), {"X", "logsv", "ybuf", "nrm"})
        assert int(row[0]) == r[4], c.name
    # the fast kernel serves N = 17..20 and Ny = 0..8 at p = 12 only; the refused shapes
    q = [(N, p, Ny) for N in (16, 17, 20, 21) for p in (11, 12, 13) for Ny in (0, 1, 8, 9)]
    for (N, p, Ny), r in zip(q, plans([f"girf {N} {p} {Ny} 0" for N, p, Ny in q])):
        assert (int(r[0]) >= 0) == (17 <= N <= 20 and p == 12 and Ny <= 8), (N, p, Ny)
    r385, rlds, r33 = (list(map(int, r)) for r in plans(["girf 32 11 0 0", "girf 2 127 0 0", "girf 2 126 0 0"]))
    assert r385[1:3] == [0, 97]                               # KT = 385: no bucket
    assert rlds[1:3] == [96, 65] and rlds[4] > LDS_CU         # 127 rows of the table: 166 KB
    assert r33[4] <= LDS_CU


def test_bign_lds_and_scratch_for_every_n(plans):
    """ccmm_bign.h on every N of the large path, at the smallest and a long TP: the padded Gram dimension, the
    four dynamic-LDS sizes (each within one CU's LDS, each the sum of the regions of its layout comment) and the SV
    scratch, whose first 3 N^2 doubles k_phi_big takes."""
    q = [(N, TP) for N in range(33, 129) for TP in (32, 768)]
    for (N, TP), row in zip(q, plans([f"bign {N} {TP}" for N, TP in q])):
        npad, astep, fin, phi, sv, scratch = map(int, row)
        assert npad == BC.astep_npad(N) and npad >= N and npad % 64 == 0, N
        assert (astep, fin, phi, sv) == (BC.astep_lds(), N * N * 8, BC.phi_lds(), BC.sv_lds(N)), N
        assert max(astep, fin, phi, sv) <= LDS_CU, N
        # what the kernels index: rows up to N - 1 of a matrix with stride 129 (128 rows hold every N), wg_gram's
        # staged chunk [32 x 129] and its 32 weights inside the same region, vec [128] after the A-step's matrix
        assert astep // 8 - 128 == phi // 8 >= max((N - 1) * 129 + N, 32 * 129 + 32), N
        assert scratch == BC.sv_scratch(N, TP) and scratch >= 3 * N * N, (N, TP)
    assert [BC.astep_npad(N) for N in (33, 64, 65, 128)] == [64, 64, 128, 128]
    assert BC.sv_lds(128) == 150528 and BC.astep_lds() == 133120  # the largest: 147 KB of 160


def test_big_solve_plan_matches_the_restatement(plans):
    """big_solve_plan (ccmm_big.h) on every sweep case of tests/bign_cases.py with and without a twin, and on the
    S120 configuration: the branch, the LDS bytes, and the pair on the LDS boundary."""
    cases = list(BC.SWEEPS) + [(120, 12, 750), (35, 2, 121)]
    q = [(c, tw) for c in cases for tw in (1, 0)]
    lines = []
    for (N, p, T), tw in q:
        K, KP, TP, ncol = BC.dims(N, p, T)
        lines.append(f"bsolve {N} {p} {K} {KP} {TP} {tw} {ncol}")
    got = {}
    for ((N, p, T), tw), row in zip(q, plans(lines)):
        K, KP, TP, ncol = BC.dims(N, p, T)
        staged, lds, base, stage = map(int, row)
        branch, want = BC.solve_plan(N, p, T, bool(tw))
        assert (staged, lds) == (int(branch == "staged"), want), (N, p, T, tw)
        assert (base, stage) == (BC.solve_lds(KP, TP), BC.stage_doubles(ncol, p, KP)), (N, p, T)
        assert lds <= LDS_CU, (N, p, T)
        got[(N, p, T), tw] = (branch, lds)
    for c, branch in BC.SWEEPS.items():
        assert got[c, 1][0] == branch and got[c, 0][0] == "none", c
    assert {b for b in BC.SWEEPS.values()} == {"staged", "kp", "lds"}
    # the LDS boundary: N = 58 stages with 1312 bytes to spare, N = 59 would need 744 bytes more than a CU has
    assert got[(58, 1, 62), 1] == ("staged", LDS_CU - 1312)
    K, KP, TP, ncol = BC.dims(59, 1, 62)
    assert BC.solve_lds(KP, TP) + BC.stage_doubles(ncol, 1, KP) * 8 == LDS_CU + 744
    assert got[(35, 9, 71), 1][0] == "staged" and BC.dims(35, 9, 71)[1] == 320  # the last staged KP
    assert got[(120, 12, 750), 1][0] == "kp"
    # a shape whose unstaged size alone exceeds a CU's LDS is not refused by the plan (the launcher's
    # hipFuncSetAttribute returns the error): TP = 2048
    r = list(map(int, plans(["bsolve 33 1 34 64 2048 1 35"])[0]))
    assert r[0] == 0 and r[1] > LDS_CU


def test_philox_words_bit_for_bit(plans):
    """tests/philox.py against the library's own host function Rng::raw on 70 counters: idx = 0, 1, 2^31,
    2^32 - 1, every block id the library uses, chains and sweeps up to 2^32 - 1, seeds below and above 2^32; and both
    against the known answers of the Random123 distribution (kat_vectors, philox4x32-10)."""
    import numpy as np
    rng = np.random.default_rng(2011)
    seeds = [0, 1, 1012023, 2**32 - 1, 2**32, (7 << 32) + 5, 2**64 - 1, 0xA4093822299F31D0]
    q = [(idx, ch, sw, blk, sd) for idx in (0, 1, 2, 3, 2**31, 2**32 - 2, 2**32 - 1) for ch, sw, blk, sd in
         [(0, 0, 9, seeds[2]), (1, 0, 10, seeds[5]), (2**32 - 1, 2**32 - 1, 1, seeds[6])]]
    q += [(int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), int(rng.integers(1, 11)),
           seeds[i % len(seeds)]) for i in range(49)]
    rows = plans([f"philox {i} {c} {s} {b} {sd & 0xFFFFFFFF} {sd >> 32}" for i, c, s, b, sd in q])
    assert len(q) >= 64
    for (i, c, s, b, sd), row in zip(q, rows):
        want = [int(w) for w in philox.raw(sd, c, s, b, i >> 1)]
        assert [int(t, 16) for t in row] == want, (i, c, s, b, hex(sd))
    # array form == scalar form
    idx = np.array([t[0] for t in q[21:]], np.uint64)
    arr = philox.raw(seeds[2], 3, 0, 9, idx >> np.uint64(1))
    for k, i in enumerate(idx):
        assert [int(w[k]) for w in arr] == [int(w) for w in philox.raw(seeds[2], 3, 0, 9, int(i) >> 1)]
    # Random123 known answers: counter and key all zero; all ones; the digits of pi
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    lib = plans([f"philox {2 * c[0]} {c[1]} {c[2]} {c[3]} {k[0]} {k[1]}" for c, k, _ in kat if c[0] < 2**31])
    for (c, k, want), row in zip([t for t in kat if t[0][0] < 2**31], lib):
        assert " ".join(row) == want
    for c, k, want in kat:
        assert " ".join(f"{int(w):08x}" for w in philox.philox4x32_10(*c, *k)) == want
    # u01 and the Box-Muller pair: (0, 1) open, 53 bits, even index cosine and odd index sine of one call
    assert philox.u01(0, 0) == 2.0**-54 and philox.u01(0xFFFFFFFF, 0xFFFFFFFF) == 1 - 2.0**-54
    assert philox.u01(0x800, 0) == 1.5 * 2.0**-53 and philox.u01(0x7FF, 0) == 2.0**-54
    x, y, z, w = philox.raw(5, 1, 0, 9, 3)
    u1, u2 = philox.u01(x, y), philox.u01(z, w)
    n6, n7 = philox.normal(5, 1, 0, 9, 6), philox.normal(5, 1, 0, 9, 7)
    assert abs(n6 * n6 + n7 * n7 + 2 * np.log(u1)) < 1e-14
    assert abs(np.arctan2(n7, n6) % (2 * np.pi) - 2 * np.pi * u2) < 1e-14
