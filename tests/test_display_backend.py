"""The display and adaptive-sampling back end (cadrays_amd/csrc/k_accumulate.h: k_accumulate, k_tile_error, k_adaptive_pick, k_tonemap,
k_hdr) against the float64 reference of tests/display_reference.py, on two sides with the SAME cases and bounds:
  cpu  the oracle (oracle/crh_oracle.c: to_ldr, accumulate_px, tile_stats, adaptive_iteration)
  gpu  the gfx950 kernels through View(0)
The oracle is a line-by-line twin of the kernels, so the bit-for-bit parity tests cannot see an error both share; this module can.

TONE MAP: the bound D.  With u = 2^-24 (one float32 rounding, relative), in the order the value is computed:
  gain   crh_exp(fl(exposure * fl(ln 2))): the argument is off by 2 u |exposure| ln 2 (the constant, the product), crh_exp by EXP_ULP
         ulps = 2 EXP_ULP u relative (test_spec_arithmetic.py pins it): d_gain = (2 |exposure| ln 2 + 2 EXP_ULP) u
  x'     fl(x * gain): d_x = d_gain + u                                                     (7.7 u at |exposure| = 3)
  mode 0 y = x':  |dy| <= d_x y
  mode 1 h(x) = N / Dn - E / F,  N = fma(x, fma(A, x, CB), DE),  Dn = fma(x, fma(A, x, B), DF):
         a constant is off by u, a product of two (CB, DE, DF) by 3 u; the inner fma adds u, the outer one u: N and Dn are off by 5 u each,
         the quotient by 11 u of N / Dn = h + E / F; the constant fl(E / F) by 3 u E / F; the subtraction adds u h:
             |dh| <= 12 u h + 14 u E / F                       (the absolute term, 0.47 u, is what is left of the cancellation near black)
         the input error d_x reaches h through d ln h / d ln x, which lies in [0, 2] (h = x (a x + b) / (F Dn) with a, b > 0);
         y = h(x') / h(w): |dy| <= (2 d_x + 12 u + d_w + u) y + 14 u (E / F) / h(w),  d_w = 12 u + 14 u (E / F) / h(w)
         (h(w) >= h(1) = 0.4011 for every white point of the grid: at most 42.2 u y + 1.17 u)
  clamp  exact
  gamma  2: z = sqrt(y), correctly rounded: |dz| <= |sqrt(y +- dy) - sqrt(y)| + u z
         2.2: crh_pow is off by POW_K u (1 + |ln z|) relative (test_spec_arithmetic.py), the exponent fl(1 / fl(2.2)) by 2 u, i.e. z by
         2 u |ln z| relative:  |dz| <= |(y +- dy)^(1 / 2.2) - z| + (POW_K (1 + |ln z|) + 2 |ln z|) u z
  byte   fma(z, 255, 0.5), one rounding of a value below 256, then truncation:  D = 255 |dz| + 256 u
D depends on where the value lies, so tonemap_bound() evaluates the chain above on the REFERENCE's quantities for every case (nothing of
the code under test enters).  Derived values: the largest D of the whole grid is 1.5e-2 byte, at the 0 | 1 boundary in filmic mode with
white point 1 and gamma 2.2 (z = 0.5 / 255, y = z^2.2 = 1.1e-6: 255 * (1 / 2.2) (z / y) * 1.17 u + 256 u); in linear mode it is at most
3.3e-4 there; from byte 8 on D < 1e-3 everywhere, and at the top of the range about 42 u * 255 / 2 = 3e-4.  test_tonemap_sweeps_are_decisive
prints and bounds the share of cases that fall within D of a rounding boundary (at most 1 % per sweep; none of the directed specials).

PICK RULE: the reference tells which draws float32 arithmetic may decide differently (display_reference.adaptive_picks).  The worst-case
bound of a float32 running sum, n_tiles 2^-24 S, is as wide as a whole tile's share of the CDF once n_tiles^2 reaches 2^24 -- at the
4160 tiles of the large case every draw would count as undecided, and the test would prove nothing.  The reference therefore uses the
smaller of that bound and an a-posteriori one that is 0 as long as every partial sum fits float32 (the all-1e3 error vector of the first
iterations: sums of 1e3 are exact), so it never excuses more than the worst-case bound does.  The large case is 520 x 512 at tile 8,
65 x 64 = 4160 tiles: above k_adaptive_pick's chunk of 4096 and no multiple of its 256 threads; no other test of this suite has more
than 4096 tiles (the widest adaptive ones are test_gpu_parity's 1080p frames of 34 x 60 = 2040).
"""
import dataclasses
import time

import numpy as np
import pytest

from cadrays_amd import scenes
from cadrays_amd.binding import BackendError
from cadrays_amd.materials import BSDF

import display_reference as R
from test_spec_arithmetic import EXP_ULP, POW_K, around, same

F32 = np.float32
EPS = 2.0 ** -24
FLT_MAX = F32(3.4028235e38)


# ================================================================================================== the two sides
class Side:
    def __init__(self, name, cls, args):
        self.name, self.cls, self.args, self.open = name, cls, args, []

    def fresh(self, sc):
        b = self.cls(*self.args).load_scene(sc)
        self.open.append(b)
        return b

    def close(self):
        for b in self.open:
            b.close()
        self.open = []


@pytest.fixture(scope="module", params=[pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def side(request, oracle_lib):
    if request.param == "cpu":
        s = Side("cpu", oracle_lib.Oracle, ())
    else:
        request.getfixturevalue("hip_lib")
        from cadrays_amd.view import View
        s = Side("gpu", View, (0,))
    yield s
    s.close()


def accum_of(b):
    """(H, W, 4) accumulator: rgb mean + sample count"""
    return b.save_accum()[0] if hasattr(b, "save_accum") else b.read_accum()


# ================================================================================================== tone map
TM_W, TM_H = 67, 61                                        # odd: the grid-stride tail of k_tonemap / k_hdr is exercised
TM_N = TM_W * TM_H * 3
MODES, GAMMAS = (0, 1), (0, 1)
EXPOSURES = (0.0, -3.0, 2.5)
WHITE_POINTS = (1.0, 4.0, 11.2, 0.0, -1.0)
CROSS_K = (0, 1, 2, 5, 17, 63, 127, 128, 200, 250, 253, 254)
SPECIALS = F32([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, -1e-45, -1e-40, -1e-3, -1.0, -FLT_MAX, -np.inf, np.nan,
                FLT_MAX, np.inf, 3.9e19, 4e19, 1e30])


def one_triangle_scene():
    pos = F32([[-1, 2, -1], [1, 2, -1], [0, 2, 1]])
    nrm = F32([[0, -1, 0]] * 3)
    tri = np.array([[0, 1, 2, 0]], np.int32)
    return scenes.Scene(pos, nrm, tri, [BSDF.CreateDiffuse(0.8)], camera=scenes.Camera(eye=(0, -3, 0)),
                        params=scenes.Params(width=TM_W, height=TM_H, max_depth=2, background=(0.2, 0.3, 0.4)), name="one_triangle")


def white_eff(mode, wp):
    """what x * gain has to reach for a full byte"""
    wp = float(F32(wp))
    return (wp if wp > 0 else 1.0) if mode == 1 else 1.0


def crossing_inputs(mode, exposure, wp, gamma22):
    """the float32 inputs next to which the reference's byte steps from k to k + 1 (255 y = k + 1/2), by bisection on the monotone reference"""
    top = white_eff(mode, wp) / 2.0 ** exposure
    lo, hi = np.zeros(len(CROSS_K)), np.full(len(CROSS_K), top)
    want = np.array(CROSS_K, np.float64) + 1.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = 255.0 * R.display_value(mid.astype(F32), mode, exposure, wp, gamma22) + 0.5 < want      # (the reference takes float32 inputs)
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return [around(F32(x), 16) for x in hi]


def tonemap_inputs(mode, exposure, wp, gamma22):
    """named segments of float32 accumulator values for one parameter set; together at most TM_N values"""
    top = white_eff(mode, wp) / 2.0 ** exposure
    r = np.random.default_rng(1000 * mode + 100 * gamma22 + int(10 * abs(exposure)) + int(F32(wp) * 7) % 97)
    dense = np.sort(r.random(6000) * 2.0 * top).astype(F32)                 # x * gain dense in [0, 2 white]
    logs = np.exp(np.linspace(np.log(1e-8), np.log(1e6), 4000)).astype(F32)
    cross = np.concatenate(crossing_inputs(mode, exposure, wp, gamma22))
    return {"dense": dense, "log": logs, "crossings": cross, "specials": SPECIALS}


def tonemap_bound(x, mode, exposure, wp, gamma22):
    """D of the module docstring for every input, in bytes: the chain of float32 roundings evaluated on the reference's quantities"""
    u = EPS
    y = R.display_value(x, mode, exposure, wp, 0) ** 2                      # the clamped value before the gamma (gamma 2 squared back)
    d_x = (2.0 * abs(exposure) * np.log(2.0) + 2.0 * EXP_ULP + 1.0) * u
    if mode == 1:
        ef = R.HABLE_E / R.HABLE_F
        hw = float(R.filmic(white_eff(mode, wp)))
        d_w = 12.0 * u + 14.0 * u * ef / hw
        dy = (2.0 * d_x + 12.0 * u + d_w + u) * y + 14.0 * u * ef / hw
    else:
        dy = d_x * y
    ylo, yhi = np.clip(y - dy, 0.0, 1.0), np.clip(y + dy, 0.0, 1.0)
    p = 1.0 / 2.2 if gamma22 else 0.5
    z = y ** p
    dz = np.maximum(yhi ** p - z, z - ylo ** p)
    if gamma22:
        with np.errstate(divide="ignore"):
            L = np.where(ylo > 0, np.abs(np.log(np.maximum(ylo, 1e-300))) * p, 0.0)      # (crh_pow(0) = 0 and crh_pow(1) = 1 are exact)
        dz = dz + (POW_K * (1.0 + L) + 2.0 * L) * u * z
    else:
        dz = dz + u * z
    return 255.0 * dz + 256.0 * u


def tonemap_grid():
    return [(e, w) for e in EXPOSURES for w in WHITE_POINTS]


def test_tonemap_reference_anchors():
    """the reference itself: the curve's closed-form values, its limit, and continuity across the x = 1 switch of its two forms"""
    A, B, C, D, E, F = R.HABLE_A, R.HABLE_B, R.HABLE_C, R.HABLE_D, R.HABLE_E, R.HABLE_F
    assert abs(float(R.filmic(0.0))) < 1e-16
    assert abs(float(R.filmic(1.0)) - ((A + C * B + D * E) / (A + B + D * F) - E / F)) < 1e-16
    assert abs(float(R.filmic(np.inf)) - (1.0 - E / F)) < 1e-16 and abs(float(R.filmic(1e300)) - (1.0 - E / F)) < 1e-12
    x = np.array([1.0 - 1e-12, 1.0, 1.0 + 1e-12])
    assert np.abs(np.diff(R.filmic(x))).max() < 1e-11
    xs = np.exp(np.linspace(np.log(1e-9), np.log(1e30), 20001))
    assert (np.diff(R.filmic(xs)) >= -4e-16).all()                          # monotone (to float64 rounding of values near 1)
    v, b = R.tonemap(F32([0, 1, np.inf, np.nan, -1, 0.25]), 0, 0.0, 1.0, 0)
    assert b.tolist() == [0, 255, 255, 0, 0, 128] and v[5] == 128.0         # sqrt(0.25) * 255 + 0.5
    v, b = R.tonemap(F32([11.2, 1e30, np.inf]), 1, 0.0, 11.2, 1)
    assert b.tolist() == [255, 255, 255]
    assert R.tonemap(F32([0.5]), 0, 1.0, 1.0, 1)[1][0] == 255 and R.tonemap(F32([0.5]), 0, -1.0, 1.0, 0)[1][0] == 128


def test_tonemap_sweeps_are_decisive():
    """the test below cannot pass by excusing cases: at most 1 % of every sweep lies within D of a rounding boundary, none of the specials"""
    worst, d_max = 0.0, 0.0
    for mode in MODES:
        for g in GAMMAS:
            for e, w in tonemap_grid():
                seg = tonemap_inputs(mode, e, w, g)
                assert sum(len(s) for s in seg.values()) <= TM_N
                for name in ("dense", "log", "specials"):
                    v, _ = R.tonemap(seg[name], mode, e, w, g)
                    D = tonemap_bound(seg[name], mode, e, w, g)
                    near = np.abs(v - np.round(v)) <= D
                    assert D.max() < 0.25                                    # (largest far below the first boundary, where v = 0.5 + a little)
                    worst = max(worst, float(near.mean())) if name != "specials" else worst
                    assert near.mean() <= (0.01 if name != "specials" else 0.0), (mode, g, e, w, name, near.mean())
                v, _ = R.tonemap(seg["crossings"], mode, e, w, g)          # the crossings really straddle their boundaries
                d_max = max(d_max, float(tonemap_bound(seg["crossings"], mode, e, w, g).max()))
                for j, k in enumerate(CROSS_K):
                    vv = v[33 * j:33 * j + 33]
                    assert vv.min() <= k + 1 <= vv.max() and (np.diff(vv) >= 0).all(), (mode, g, e, w, k)
    print(f"tone map: largest D at a rounding boundary {d_max:.3e} byte; largest share of a sweep within D of a boundary {worst:.4%}")
    assert d_max < 2e-2


@pytest.fixture(scope="module")
def tm_backend(side):
    return side.fresh(one_triangle_scene())


@pytest.mark.parametrize("gamma22", GAMMAS)
@pytest.mark.parametrize("mode", MODES)
def test_tonemap_against_reference(side, tm_backend, mode, gamma22):
    b = tm_backend
    base = one_triangle_scene().params
    b.set_spec(display_gamma22=gamma22)
    excused = total = 0
    for e, w in tonemap_grid():
        what = (side.name, mode, gamma22, e, w)
        seg = tonemap_inputs(mode, e, w, gamma22)
        flat = np.zeros(TM_N, F32)
        at, where = 0, {}
        for name, s in seg.items():
            flat[at:at + len(s)] = s
            where[name] = slice(at, at + len(s))
            at += len(s)
        rgba = np.ones((TM_H, TM_W, 4), F32)
        rgba[..., :3] = flat.reshape(TM_H, TM_W, 3)
        b.set_params(dataclasses.replace(base, tonemap_mode=mode, exposure=e, white_point=w))
        b.load_accum(rgba, 1)
        got = b.read_ldr().reshape(-1).astype(np.int64)
        if side.name == "gpu":                                              # the asynchronous read-back runs the same kernel on another stream
            b.read_ldr_begin()
            assert np.array_equal(b.read_ldr_end().reshape(-1), got), what
        assert same(b.read_hdr().reshape(-1), flat).all(), what             # k_hdr: the injected values bit for bit, NaN as NaN
        v, ref = R.tonemap(flat, mode, e, w, gamma22)
        D = tonemap_bound(flat, mode, e, w, gamma22)
        near = np.abs(v - np.round(v)) <= D
        ref = ref.astype(np.int64)
        bad = np.where(near, np.abs(got - ref) > 1, got != ref)
        assert not bad.any(), (what, flat[bad][:8], got[bad][:8], ref[bad][:8], v[bad][:8])
        sw = np.r_[where["dense"], where["log"]]
        excused += int(near[sw].sum()); total += len(sw)
        assert not near[where["specials"]].any()
        # non-decreasing along every sorted sweep (a seam in crh_pow / hable would show); over ALL inputs in order, neighbouring floats at the
        # crossings included, a step down is possible only between two values that both lie within D of the same boundary (the filmic
        # chain of six roundings is not monotone to the last bit; the linear one is, and is held to it)
        for name in ("dense", "log"):
            assert (np.diff(got[where[name]]) >= 0).all(), (what, name)
        allx = flat[:at]
        keep = np.isfinite(allx) & (allx >= 0)
        order = np.argsort(allx[keep], kind="stable")
        down = np.diff(got[:at][keep][order]) < 0
        both_near = near[:at][keep][order][1:] & near[:at][keep][order][:-1]
        assert not (down & ~both_near).any() and (mode == 1 or not down.any()), what
        for j, k in enumerate(CROSS_K):
            c = got[where["crossings"]][33 * j:33 * j + 33]
            assert set(c.tolist()) <= {k, k + 1}, (what, k, c)
        # exact anchors
        gx = np.where(np.isnan(flat) | (flat < 0), 0.0, flat.astype(np.float64)) * 2.0 ** float(F32(e))
        assert (got[(gx == 0)] == 0).all(), what                            # 0, -0, NaN, negatives, -inf
        full = gx >= white_eff(mode, w)
        assert full[where["specials"]][-5:].all()                           # FLT_MAX, +inf, 3.9e19, 4e19, 1e30: all beyond every white point
        assert (got[full] == 255).all(), (what, flat[full & (got != 255)][:8], got[full & (got != 255)][:8])
    print(f"tone map {side.name} mode {mode} gamma22 {gamma22}: {excused} of {total} sweep cases within D of a rounding boundary ({excused / total:.4%})")
    assert excused <= 0.01 * total


def test_load_accum_contract(side):
    """orc_load_accum / crh_load_accum: accumulator and iteration counter are replaced; refused while adaptive sampling is on"""
    b = side.fresh(one_triangle_scene())
    r = np.random.default_rng(5)
    rgba = r.random((TM_H, TM_W, 4), dtype=F32)
    rgba[..., 3] = 3.0
    b.load_accum(rgba, 3)
    assert np.array_equal(accum_of(b), rgba) and np.array_equal(b.read_hdr(), rgba[..., :3])
    b.render(1)                                                             # goes on from sample 3: (3 mean + s) / 4
    a = accum_of(b)
    assert (a[..., 3] == 4.0).all()
    f = side.fresh(one_triangle_scene())
    f.render_tiles(np.arange(f.n_tiles()), 3, 1)
    want = (3.0 * rgba[..., :3].astype(np.float64) + f.read_hdr()) / 4.0
    assert np.abs(a[..., :3] - want).max() <= 4 * EPS * max(1.0, float(f.read_hdr().max()))
    b.set_adaptive(True, 2)
    with pytest.raises(BackendError):
        b.load_accum(rgba, 3)
    b.set_adaptive(False, 2)
    b.load_accum(rgba, 3)


# ================================================================================================== running mean, variance, picks
W, H, TS = 80, 48, 32                                      # 3 x 2 tiles: the last column (16 wide) and row (16 high) are ragged
N_S = 48
ALL = np.arange(6, dtype=np.uint32)


def box():
    return scenes.cornell_box(True, W, H)


_S = {}


def sample_stack(side):
    """S[k]: radiance of sample k alone, from a context of its own (a mean of one sample IS the sample: fma(v - 0, 1, 0)); made once per side"""
    if side.name in _S:
        return _S[side.name]
    t0 = time.time()
    out = np.empty((N_S, H, W, 3), np.float64)
    for k in range(N_S):
        b = side.cls(*side.args).load_scene(box())
        b.render_tiles(ALL, k, 1)
        out[k] = b.read_hdr()
        if k == 0:
            assert (accum_of(b)[..., 3] == 1.0).all()
        b.close()
    assert np.isfinite(out).all() and out.max() > 1.0 and (out.std(0) > 0).mean() > 0.25     # a picture with noise in it, not a constant
    print(f"S[{N_S}] on {side.name}: {time.time() - t0:.2f} s")
    out.setflags(write=False)
    _S[side.name] = out
    return out


@pytest.fixture(scope="module")
def S(side):
    return sample_stack(side)


def check_mean(b, S_, first, ns, tiles=ALL, clampv=0.0, what=None):
    """accumulator of `b` == mean(S[first : first + ns]) on `tiles` within the recurrence bound 2 ns 2^-24 max_k |S[k]|, counts == ns; nothing elsewhere"""
    a = accum_of(b).astype(np.float64)
    s = S_[first:first + ns]
    if clampv > 0:
        s = np.minimum(s, clampv)
    want, tol = s.mean(0), 2.0 * ns * EPS * np.abs(s).max(0)
    inside = np.zeros((H, W), bool)
    for t in tiles:
        inside[R.tile_rect(int(t), W, H, TS)] = True
    assert (a[inside, 3] == ns).all() and (a[~inside] == 0).all(), what
    err = np.abs(a[..., :3] - want)[inside]
    assert (err <= tol[inside]).all(), (what, first, ns, float((err - tol[inside]).max()))
    assert np.array_equal(b.read_hdr().astype(np.float64)[inside], a[inside, :3]), what


# batches of 8, 24 and 40 take k_accumulate's LDS path (runs of >= 8 consecutive samples per pixel), the others the per-lane path
@pytest.mark.parametrize("first,ns", [(0, 8), (3, 8), (0, 24), (5, 40), (0, 12), (7, 7), (1, 1)])
def test_running_mean(side, S, first, ns):
    b = side.fresh(box())
    b.render_tiles(ALL, first, ns)
    check_mean(b, S, first, ns, what=side.name)


def test_running_mean_consecutive_calls_subset_and_clamp(side, S):
    b = side.fresh(box())
    b.render_tiles(ALL, 0, 8)
    b.render_tiles(ALL, 8, 5)
    check_mean(b, S, 0, 13, what="(0, 8) then (8, 5)")
    b = side.fresh(box())
    b.render_tiles(np.array([1, 4], np.uint32), 0, 8)
    check_mean(b, S, 0, 8, tiles=[1, 4], what="tiles 1 and 4 only")
    sc = box()
    b = side.fresh(dataclasses.replace(sc, params=dataclasses.replace(sc.params, radiance_clamp=2.0)))
    assert (S[:24] > 2.0).any()                                             # the clamp has something to do
    b.render_tiles(ALL, 0, 24)
    check_mean(b, S, 0, 24, clampv=2.0, what="radiance_clamp 2")
    b.render_tiles(ALL, 24, 7)
    check_mean(b, S, 0, 31, clampv=2.0, what="radiance_clamp 2, per-lane path")


@pytest.mark.gpu
def test_running_mean_split_batches_gpu(hip_lib):
    """crh_render_tiles cuts a batch that exceeds the path budget into tile groups and sample ranges of budget / (tiles * 1024) samples, each a
    batch of its own (crh_schedule.cpp render_impl); sub-ranges of ONE traced batch that start off a multiple of 8 -- the `first_sample & ~7u`
    start of the LDS loop -- come from the look-ahead (crh_set_lookahead: 24 frames traced at once, folded in as the Redraw()s ask)"""
    from cadrays_amd.view import View
    side = Side("gpu", View, (0,))                                          # (the path budget and the look-ahead are the product's: the oracle has neither)
    S = sample_stack(side)
    for budget, why in ((6 * 1024 * 5, "24 samples as 5 + 5 + 5 + 5 + 4"), (6 * 1024 * 8, "as 8 + 8 + 8"), (4 * 1024, "tile groups 4 + 2, one sample each")):
        b = side.fresh(box())
        b.set_path_budget(budget)
        assert b.get_path_budget() == budget < 6 * 1024 * 24                # the batch cannot be traced in one piece
        b.render_tiles(ALL, 0, 24)
        check_mean(b, S, 0, 24, what=why)
    b = side.fresh(box())
    b.set_lookahead(24)
    done = 0
    for n in (5, 7, 12):                                                    # [0, 5), [5, 12), [12, 24) of one batch of 24
        b.render(n)
        done += n
        check_mean(b, S, 0, done, what=f"look-ahead 24, {done} folded in")
    assert b.save_accum()[1] == 24
    side.close()


def test_variance_estimate_and_tile_error(side, S):
    b = side.fresh(box())
    b.set_adaptive(True, 3)
    b.render(1)
    err, cnt = b.tile_stats()
    assert cnt.max() == 1 and (err == F32(1e3)).all()                       # fewer than two samples: exactly 1e3
    b.render(19)
    err, cnt = b.tile_stats()
    a = accum_of(b).astype(np.float64)
    assert 2 <= cnt.max() <= N_S and cnt.sum() <= 60, cnt
    for t in range(6):
        px = a[R.tile_rect(t, W, H, TS)]
        n = int(cnt[t])
        assert (px[..., 3] == n).all(), (t, n)                              # every pixel of the tile has the tile's count
        if n:                                                               # ... and the mean of the uniform sequence's first n samples: tile t's
            s = S[:n][(slice(None),) + R.tile_rect(t, W, H, TS)]            # sample k is frame k, whenever it was drawn
            assert (np.abs(px[..., :3] - s.mean(0)) <= 2.0 * n * EPS * np.abs(s).max(0)).all(), (t, n)
    val, lo, hi = R.tile_error_bounds(S, cnt, W, H, TS)
    wide = 256.0 * EPS                                                      # the 256-term summation of the tile's pixel errors
    few = cnt < 2
    assert (err[few] == F32(1e3)).all()
    assert (err >= lo * (1.0 - wide)).all() and (err <= hi * (1.0 + wide)).all(), (err, lo, hi)
    rel = (hi - lo)[val > 0] / val[val > 0]                                # (a tile of background only: value 0)
    print(f"tile error {side.name}: counts {cnt.tolist()}, brackets {np.sort(rel)} of the value")
    assert rel.min() < 1e-3                                                 # the brackets are narrow enough to tell a wrong estimator


def constant_scene():
    """nothing in view: every sample of every pixel is the background"""
    sc = one_triangle_scene()
    pos = sc.pos.copy(); pos[:, 1] = -10.0                                  # behind the camera
    return dataclasses.replace(sc, pos=pos, params=scenes.Params(width=W, height=H, tile_size=TS, max_depth=2, background=(0.3, 0.5, 0.2)))


def run_pick_iterations(b, per_iter, iters, pick0=0, max_undecided=0.0):
    """every iteration: the tiles whose count rose are the ones the reference draws from the error vector read just before it"""
    undecided = draws_n = 0
    for it in range(iters):
        err, cnt = b.tile_stats()
        b.render(1)
        _, cnt2 = b.tile_stats()
        step = cnt2.astype(np.int64) - cnt
        assert set(np.unique(step).tolist()) <= {0, 1}, (it, np.unique(step))
        picked = set(np.flatnonzero(step).tolist())
        tiles, draws = R.adaptive_picks(err, pick0, per_iter)
        pick0 += per_iter
        und = [d for d in draws if d["undecided"]]
        undecided += len(und); draws_n += len(draws)
        sure = {d["tile"] for d in draws if not d["undecided"]}
        assert sure <= picked, (it, sorted(sure - picked)[:8])
        for t in picked - sure:
            assert any(d["lo"] <= t <= d["hi"] for d in und), (it, t)
        for d in und:
            assert any(t in picked for t in range(d["lo"], d["hi"] + 1)), (it, d)
        if not und:
            assert picked == tiles
    assert undecided <= max_undecided * draws_n, (undecided, draws_n)
    return undecided, draws_n


def test_pick_rule_small(side):
    b = side.fresh(box())
    b.set_adaptive(True, 5)
    err, cnt = b.tile_stats()
    assert (err == F32(1e3)).all() and (cnt == 0).all()                     # the equal-weights start
    und, n = run_pick_iterations(b, 5, 12)
    err, cnt = b.tile_stats()
    assert (err < 1e3).all() and len(set(err.tolist())) >= 4               # ... and real, unequal estimates by the end
    print(f"pick rule small {side.name}: {und} of {n} draws undecided; counts {cnt.tolist()}")


def test_pick_rule_uniform_branch(side):
    """no estimate to go by (sum of the errors 0: two equal samples everywhere): tile floor(u n_tiles)"""
    b = side.fresh(constant_scene())
    b.set_adaptive(True, 5)
    b.render_tiles(ALL, 0, 2)
    err, cnt = b.tile_stats()
    assert (err == 0).all() and (cnt == 2).all()
    hdr = b.read_hdr()
    assert (hdr == F32([0.3, 0.5, 0.2])).all()
    und, n = run_pick_iterations(b, 5, 4)
    assert (b.tile_stats()[0] == 0).all()
    print(f"pick rule uniform branch {side.name}: {und} of {n} draws undecided")


def test_pick_rule_above_one_chunk(side):
    sc = scenes.cornell_box(False, 520, 512)
    sc = dataclasses.replace(sc, params=dataclasses.replace(sc.params, tile_size=8))
    b = side.fresh(sc)
    assert b.n_tiles() == 4160
    b.set_adaptive(True, 512)
    und, n = run_pick_iterations(b, 512, 4, max_undecided=0.01)
    _, cnt = b.tile_stats()
    a = accum_of(b)
    per_px = a[..., 3].reshape(64, 8, 65, 8)
    assert (per_px == cnt.reshape(64, 1, 65, 1)).all()                      # the ordered compaction sent every picked tile's pixels, and no others, one sample
    assert cnt[4096:].sum() > 0 and cnt[:4096].sum() > 0                    # tiles of the second chunk among them
    print(f"pick rule 4160 tiles {side.name}: {und} of {n} draws undecided; {int(cnt.sum())} samples on {int((cnt > 0).sum())} tiles")
