"""Display state without a restart and auto exposure on the device (include/cadrays_hip.h: crh_set_display, crh_set_auto_exposure,
crh_measure_exposure, crh_meter_from_histogram; kernels in cadrays_amd/csrc/k_meter.h) against the numpy restatement of
tests/metering_reference.py.

What is compared and how tightly:
  rule, host     crh_meter_from_histogram == the restatement, bit for bit (integers, one float64 division, one float32 rounding, crh_exp as the CPU
                 build evaluates it: the checker's math hook fn 1)
  histogram      synthetic accumulators of single-channel pixels, where the luminance is ONE float32 rounding: every count equal
  rendered       float64 luminance; the kernel's three float32 roundings keep its value within 3 * 2^-24 * (1 + 2^-20) relative, a pixel closer than that
                 to a bin edge may fall on either side: every count between its decided number and that plus its undecided neighbours; at most
                 0.1 % of the pixels may be undecided (expected: 6 * 2^-24 of a bin that is at least 14 % wide, i.e. a few in a million)
  rule, device   crh_measure_exposure's exposure / white point / bin == crh_meter_from_histogram of its own histogram, bit for bit
  end to end     bytes with auto exposure on (synchronous and asynchronous read-out) == bytes with it off after crh_set_display(measured values)
  no restart     HDR image, frame counter and ray counters equal those of a context that never heard of any of this

Sizes: 61 x 37 and 131 x 75 (odd, no multiple of the workgroup; one / three workgroups of k_luma_histogram) and one frame of more than
grid x 256 x 16 pixels: the histogram kernel gets one workgroup per 4096 pixels up to the device's streaming grid (4 per compute unit), beyond which
every thread takes further rounds of its grid-stride loop.
"""
import dataclasses

import numpy as np
import pytest

from cadrays_amd import scenes
from cadrays_amd.binding import BackendError
from cadrays_amd.materials import BSDF

import metering_reference as R
from test_two_level import object_scene

F32, U32 = np.float32, np.uint32
FLT_MAX = F32(3.4028235e38)


# ================================================================================================== the rule on the host (no GPU)
@pytest.fixture(scope="module")
def crh_exp(oracle_lib):
    return lambda x: oracle_lib.math_fn(1, np.array([x], F32))[0][0]


def same_bits(a, b):
    return np.array(a, F32).view(U32) == np.array(b, F32).view(U32)


def check_rule(hip_lib, crh_exp, hist, exposure_in=0.0, white_in=1.0, **params):
    from cadrays_amd.view import meter_from_histogram
    got = meter_from_histogram(hist, exposure_in, white_in, **params)
    want = R.meter(hist, crh_exp, exposure_in, white_in, **params)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], (got, want, params)
    return got


def one_bin(i, n=1000):
    h = np.zeros(256, U32); h[i] = n
    return h


def test_defaults_match_the_mirror(hip_lib):
    import ctypes as C
    from cadrays_amd import abi
    p = abi.crh_meter_params()
    hip_lib.crh_meter_defaults.restype = None
    hip_lib.crh_meter_defaults(C.byref(p))
    assert p.key_stops == float(F32(np.log2(0.18))) == abi.METER_DEFAULTS["key_stops"]
    assert (p.min_stops, p.max_stops, p.white_permille, p.white_min, p.white_max, tuple(p.rect)) == (-10.0, 10.0, 990, 1.0, 10.0, (0, 0, 0, 0))


def test_rule_random_histograms(hip_lib, crh_exp):
    r = np.random.default_rng(11)
    for k in range(200):
        h = r.integers(0, 2 ** int(r.integers(1, 33)), 256, dtype=np.uint64).astype(U32)
        h[r.random(256) < r.random()] = 0                                   # sparse ones too
        lo, hi = int(r.integers(0, 200)), int(r.integers(56, 256))
        if k % 3 == 0:
            h[:lo] = 0; h[hi:] = 0                                           # a band, as an image has
        check_rule(hip_lib, crh_exp, h, exposure_in=float(r.normal()), white_in=float(1 + 5 * r.random()),
                   white_permille=int(r.integers(0, 1001)), key_stops=float(r.normal(-2.5, 2)))


def test_rule_directed_histograms(hip_lib, crh_exp):
    zero = np.zeros(256, U32)
    assert check_rule(hip_lib, crh_exp, zero, 1.25, 3.5) == (F32(1.25), F32(3.5), 0)                 # nothing at all: the display values
    assert check_rule(hip_lib, crh_exp, one_bin(0), -0.5, 2.0) == (F32(-0.5), F32(2.0), 0)           # only black pixels: nothing lit
    for i in (1, 2, 100, 127, 128, 129, 200, 254):
        e, w, b = check_rule(hip_lib, crh_exp, one_bin(i))
        assert b == i
    e, w, b = check_rule(hip_lib, crh_exp, one_bin(255))                                              # only overflow: clamped, bin 255's upper edge
    assert e == F32(-10.0) and b == 255
    check_rule(hip_lib, crh_exp, one_bin(255), min_stops=-40.0)
    h = one_bin(131, 2 ** 28); check_rule(hip_lib, crh_exp, h)                                        # a whole 2^28-pixel target in one bin
    h[7] = 2 ** 28; h[250] = 2 ** 28; check_rule(hip_lib, crh_exp, h)
    full = np.full(256, 2 ** 32 - 1, np.uint64).astype(U32); check_rule(hip_lib, crh_exp, full)     # sums far beyond 32 bits


def test_rule_white_permille(hip_lib, crh_exp):
    h = np.zeros(256, U32); h[100] = 1000; h[120] = 9; h[140] = 1
    assert check_rule(hip_lib, crh_exp, h, 0.0, 4.5, white_permille=0)[1:] == (F32(4.5), 0)          # 0: the display white point stays
    assert check_rule(hip_lib, crh_exp, h, white_permille=1)[2] == 100                               # target ceil(1.01) = 2
    assert check_rule(hip_lib, crh_exp, h, white_permille=1000)[2] == 140                            # every pixel: the last lit bin
    assert check_rule(hip_lib, crh_exp, h, white_permille=990)[2] == 100                             # ceil(999.9) = 1000 is reached in bin 100
    assert check_rule(hip_lib, crh_exp, h, white_permille=991)[2] == 120                             # ceil(1000.91) = 1001 is not
    assert check_rule(hip_lib, crh_exp, one_bin(90, 1), white_permille=1)[2] == 90                   # N = 1: target 1, not 0


def test_rule_every_clamp(hip_lib, crh_exp):
    dark, bright, mid = one_bin(20), one_bin(230), one_bin(125)
    assert check_rule(hip_lib, crh_exp, dark)[0] == F32(10.0)                                        # max_stops
    assert check_rule(hip_lib, crh_exp, bright)[0] == F32(-10.0)                                     # min_stops
    assert check_rule(hip_lib, crh_exp, dark, max_stops=3.25)[0] == F32(3.25)
    assert check_rule(hip_lib, crh_exp, bright, min_stops=-1.5)[0] == F32(-1.5)
    e, w, _ = check_rule(hip_lib, crh_exp, mid)                                                      # no clamp on the exposure ...
    assert -10 < e < 10 and w == F32(1.0)                                                            # ... one bin: its upper edge lands below white_min
    assert check_rule(hip_lib, crh_exp, mid, white_min=0.01, white_max=0.02)[1] == F32(0.02)         # white_max
    h = mid.copy(); h[145] = 100
    e, w, b = check_rule(hip_lib, crh_exp, h, white_permille=1000)                                   # neither white clamp
    assert b == 145 and 1.0 < w < 10.0
    assert check_rule(hip_lib, crh_exp, h, white_permille=1000, white_max=1.5)[1] == F32(1.5)
    assert check_rule(hip_lib, crh_exp, dark, key_stops=150.0, max_stops=200.0, white_permille=1000)[1] == F32(10.0)  # the gain overflows to +inf: white_max


def test_rule_rejects_bad_params(hip_lib):
    from cadrays_amd.view import meter_from_histogram
    h = one_bin(100)
    for bad in (dict(key_stops=np.nan), dict(min_stops=np.nan), dict(max_stops=np.inf), dict(white_min=np.nan), dict(white_max=-np.inf),
                dict(min_stops=1.0, max_stops=0.0), dict(white_min=3.0, white_max=2.0), dict(white_permille=1001)):
        with pytest.raises(BackendError):
            meter_from_histogram(h, **bad)
    for bad_in in ((np.nan, 1.0), (0.0, np.inf)):
        with pytest.raises(BackendError):
            meter_from_histogram(h, *bad_in)
    with pytest.raises(ValueError):
        meter_from_histogram(h, no_such_field=1)


def test_reference_bins_are_what_the_rule_text_says():
    """the restatement itself: four bins per octave from 2^-32, mantissas 1 / 1.25 / 1.5 / 1.75, denormals in 1, overflow in 255"""
    assert R.lower_edge(1) == F32(2.0 ** -32) and R.lower_edge(2) == F32(1.25 * 2.0 ** -32) and R.lower_edge(4) == F32(1.75 * 2.0 ** -32) and R.lower_edge(5) == F32(2.0 ** -31)
    assert R.lower_edge(129) == F32(1.0) and R.lower_edge(255) == F32(1.5 * 2.0 ** 31) and R.lower_edge(256) == F32(1.75 * 2.0 ** 31)
    l = F32([0.0, 1e-45, 1e-38, 2.0 ** -33, 2.0 ** -32, 0.18, 0.99999994, 1.0, 1.25, 2.0, 1.75 * 2.0 ** 31, 3e38, np.inf])
    assert R.bin_of(l).tolist() == [0, 1, 1, 1, 1, 118, 128, 129, 130, 133, 255, 255, 255]


# ================================================================================================== GPU: the histogram is exact
def flat_scene(w, h):
    pos = F32([[-1, 2, -1], [1, 2, -1], [0, 2, 1]])
    return scenes.Scene(pos, F32([[0, -1, 0]] * 3), np.array([[0, 1, 2, 0]], np.int32), [BSDF.CreateDiffuse(0.8)], camera=scenes.Camera(eye=(0, -3, 0)),
                        params=scenes.Params(width=w, height=h, max_depth=2, background=(0.2, 0.3, 0.4)), name="one_triangle")


@pytest.fixture(scope="module")
def view(hip_lib):
    from cadrays_amd.view import View
    v = View(0).load_scene(flat_scene(61, 37))
    yield v
    v.close()


def large_size():
    """more pixels than grid x 256 x 16, the grid being the device's streaming grid of 4 workgroups per compute unit (crh_context.h `grid`)"""
    import torch
    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    w = 2051
    return w, (grid * 256 * 16) // w + 3


SIZES = [(61, 37), (131, 75), "large"]


def sized(view, size):
    w, h = large_size() if size == "large" else size
    if (view.width, view.height) != (w, h):
        view.ChangeRenderingParams(width=w, height=h)
    return w, h


def edge_values():
    """for every lower edge E of bins 1 .. 255 and the upper edge of 255: the smallest float32 v with fl(0.7152f * v) >= E, and the float before it"""
    E = R.lower_edge(np.arange(1, 257))
    v = (E.astype(np.float64) / np.float64(R.W_G)).astype(F32)
    for _ in range(4):
        v = np.nextafter(v, F32(0))                      # start safely below ...
    for _ in range(12):                                  # ... and walk up to the first value that reaches the edge
        v = np.where((R.W_G * v).astype(F32) >= E, v, np.nextafter(v, F32(np.inf)))
    below = np.nextafter(v, F32(0))
    assert ((R.W_G * v).astype(F32) >= E).all() and ((R.W_G * below).astype(F32) < E).all()
    return np.concatenate([v, below])


def special_pixels():
    nan, inf, den = F32(np.nan), F32(np.inf), F32(1e-40)
    return F32([[nan, 0, 0, 1], [0, nan, 0, 2], [-1, 0, 0, 1], [0, 0, -1, 1], [-0.0, -0.0, -0.0, 1], [0, 0, 0, 1], [inf, 0, 0, 1], [0, 0, inf, 1], [-inf, 0, 0, 1],
                [nan, 0.5, -3, 1], [-inf, nan, 0.25, 1],
                [FLT_MAX, 0, 0, 1], [0, FLT_MAX, 0, 7], [0, 0, FLT_MAX, 1], [0, den, 0, 1], [den, 0, 0, 1], [0, 0, 1e-45, 1], [0, 2.0 ** -31, 0, 1],
                [1, 2, 3, 0], [1, 2, 3, -0.0], [0.5, 0, 0, -1], [0, 0.5, 0, nan], [nan, nan, nan, 0], [0, 1, 0, 1e-45], [0, 1, 0, inf]])


def ramp_image(w, h, seed):
    """the 512 edge values in green, the specials, then random single-channel pixels over the whole range of the bins, every 13th unsampled"""
    r = np.random.default_rng(seed)
    n = w * h
    a = np.zeros((n, 4), F32)
    ch = r.integers(0, 3, n)
    a[np.arange(n), ch] = np.exp2(r.uniform(-36, 34, n)).astype(F32)
    a[:, 3] = r.integers(1, 5, n)
    a[::13, 3] = 0
    ev, sp = edge_values(), special_pixels()
    k = len(ev)
    a[:k] = 0; a[:k, 1] = ev; a[:k, 3] = 1
    a[k:k + len(sp)] = sp
    a = a[r.permutation(n)] if n < 100000 else np.roll(a, 977, axis=0)      # the edges anywhere in the frame, not in its first workgroup
    return a.reshape(h, w, 4)


def measure(view, **params):
    m = view.measure_exposure(**params)
    assert m["n_lit"] == int(m["hist"][1:].astype(np.int64).sum())
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_histogram_constant_image(view, size):
    """the contention case: every lane of every wavefront on one LDS word"""
    w, h = sized(view, size)
    a = np.zeros((h, w, 4), F32); a[..., 0] = 0.5; a[..., 3] = 3
    view.load_accum(a, 3)
    m = measure(view)
    want = np.zeros(256, np.int64); want[int(R.bin_of(np.array([R.W_R * F32(0.5)]))[0])] = w * h
    assert np.array_equal(m["hist"], want) and m["n_unsampled"] == 0 and m["n_lit"] == w * h
    a[..., 3] = 0
    view.load_accum(a, 0)
    m = measure(view)
    assert not m["hist"].any() and m["n_unsampled"] == w * h


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_histogram_ramp_specials_and_rectangles(view, size):
    w, h = sized(view, size)
    a = ramp_image(w, h, 5)
    view.load_accum(a, 1)
    want, uns = R.histogram_single(a)
    if size != "large":
        assert (want[1:] > 0).all()                       # every bin is hit (both sides of all 255 edges)
    m = measure(view)
    assert np.array_equal(m["hist"], want), np.nonzero(m["hist"] != want)
    assert m["n_unsampled"] == uns and int(m["hist"].astype(np.int64).sum()) + uns == w * h
    for rect in ((3, 5, w - 8, h - 6), (1, 1, 2, 2), (w - 1, 0, w, h), (0, h - 3, w, h), (7, 3, w + 100, h + 100)):      # odd offsets; one pixel; last column; full-width rows; cut to the frame
        want, uns = R.histogram_single(a, (rect[0], rect[1], min(rect[2], w), min(rect[3], h)))
        m = measure(view, rect=rect)
        assert np.array_equal(m["hist"], want), rect
        assert m["n_unsampled"] == uns and int(m["hist"].astype(np.int64).sum()) + uns == (min(rect[2], w) - rect[0]) * (min(rect[3], h) - rect[1]), rect
    for rect in ((5, 5, 5, 9), (9, 4, 3, 20), (w + 5, 0, w + 9, 4)):      # empty, inverted, wholly outside: the whole frame
        assert np.array_equal(measure(view, rect=rect)["hist"], R.histogram_single(a)[0]), rect


# ================================================================================================== GPU: rendered image, the rule on the device, the bytes
@pytest.fixture(scope="module")
def rendered(hip_lib):
    """the small object scene with three samples per pixel; tests leave frames and display state as they found them or say so"""
    from cadrays_amd.view import View
    v = View(0).load_scene(object_scene())
    v.render(3)
    yield v
    v.close()


UNDECIDED_CAP = 1e-3


@pytest.mark.gpu
def test_histogram_of_a_rendered_image(rendered):
    acc, _ = rendered.save_accum()
    for rect in ((0, 0, 0, 0), (5, 11, 90, 77)):
        lo, hi, uns, share = R.histogram_bounds(acc, rect)
        print(f"rect {rect}: undecided share {share:.3e} (cap {UNDECIDED_CAP:.0e}); lit bins {np.count_nonzero(lo[1:])}")
        assert share <= UNDECIDED_CAP, share
        m = measure(rendered, rect=rect)
        assert (lo <= m["hist"]).all() and (m["hist"] <= hi).all(), np.nonzero((lo > m["hist"]) | (m["hist"] > hi))
        assert m["n_unsampled"] == uns
    assert np.count_nonzero(lo[1:]) >= 20                 # a real image: the histogram is not one spike


PARAM_SETS = [dict(), dict(white_permille=0), dict(white_permille=1000, white_max=100.0), dict(key_stops=0.0, white_permille=500, white_min=0.001),
              dict(max_stops=-3.0), dict(min_stops=4.0), dict(rect=(5, 11, 90, 77), white_permille=10)]


@pytest.mark.gpu
def test_rule_on_the_device_equals_the_host_entry_point(rendered, view):
    from cadrays_amd.view import meter_from_histogram
    w, h = sized(view, (131, 75))
    view.load_accum(ramp_image(w, h, 9), 1)
    dark = np.zeros((h, w, 4), F32); dark[..., 3] = 1
    for v, disp in ((rendered, (1, 0.75, 3.0)), (view, (0, -1.5, 0.5))):
        v.set_display(*disp)
        for params in PARAM_SETS:
            m = v.measure_exposure(**params)
            e, wp, b = meter_from_histogram(m["hist"], disp[1], disp[2], **params)
            assert same_bits(m["exposure"], e) and same_bits(m["white_point"], wp) and m["white_bin"] == b, (params, m, (e, wp, b))
    view.load_accum(dark, 1)                              # nothing lit: the display values come back
    m = view.measure_exposure()
    assert (m["exposure"], m["white_point"], m["white_bin"], m["n_lit"]) == (F32(-1.5), F32(0.5), 0, 0) and m["hist"][0] == w * h
    rendered.set_display(0, 0.0, 1.0); view.set_display(0, 0.0, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("gamma22", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_auto_exposure_bytes_equal_the_manual_setting(hip_lib, mode, gamma22):
    from cadrays_amd.view import View
    sc = dataclasses.replace(object_scene(), spec=dict(display_gamma22=gamma22))
    v = View(0).load_scene(sc)
    try:
        v.render(3)
        for selection in (False, True):
            if selection:
                flags = np.zeros(len(sc.obj_xform), np.uint8); flags[[3, 5]] = 1
                v.set_selection(flags, (255, 160, 0), 64); v.set_hover(4)
            for params in (dict(), dict(rect=(9, 7, 80, 70), white_permille=900, key_stops=-1.0)):
                v.set_display(mode, 0.5, 2.0)
                plain = v.read_ldr()
                v.set_auto_exposure(True, **params)
                assert v.get_display() == dict(tonemap_mode=mode, exposure=0.5, white_point=2.0, auto_on=True)
                sync = v.read_ldr()
                v.read_ldr_begin(); v.read_ldr_begin()                      # both read-back slots
                a0, a1 = v.read_ldr_end(), v.read_ldr_end()
                m = v.measure_exposure(**params)
                assert m["exposure"] != F32(0.5) and m["white_point"] != F32(2.0)      # the metering has something to say here
                v.set_auto_exposure(False)
                assert not v.get_display()["auto_on"] and np.array_equal(v.read_ldr(), plain)      # off again: the bytes of before
                v.set_display(mode, m["exposure"], m["white_point"])
                manual = v.read_ldr()
                assert np.array_equal(sync, manual) and np.array_equal(a0, manual) and np.array_equal(a1, manual)
                assert not np.array_equal(manual, plain)
    finally:
        v.close()


@pytest.mark.gpu
def test_display_calls_restart_nothing(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene()
    n, k = 3, 2
    a, b = View(0).load_scene(sc), View(0).load_scene(sc)
    c = View(0).load_scene(dataclasses.replace(sc, params=dataclasses.replace(sc.params, tonemap_mode=1, exposure=1.25, white_point=3.0)))
    try:
        for v in (a, b, c):
            v.set_lookahead(4)                            # samples traced ahead are pending while the display calls arrive
            for _ in range(n):
                v.render(1)
        a.set_display(1, 1.25, 3.0)
        assert a.get_display() == dict(tonemap_mode=1, exposure=1.25, white_point=3.0, auto_on=False)
        a.set_auto_exposure(True)
        a.measure_exposure()
        metered = a.read_ldr()
        a.set_auto_exposure(False)
        for v in (a, b, c):
            for _ in range(k):
                v.render(1)
        (acc_a, fa), (acc_b, fb) = a.save_accum(), b.save_accum()
        assert fa == fb == n + k and np.array_equal(acc_a.view(U32), acc_b.view(U32))
        assert np.array_equal(a.read_hdr().view(U32), b.read_hdr().view(U32))
        sa, sb = a.stats(), b.stats()
        assert all(sa[f] == sb[f] for f in ("rays_nearest", "rays_any", "shaded_hits", "samples")), (sa, sb)      # nothing traced ahead was thrown away
        ldr = a.read_ldr()
        assert np.array_equal(ldr, c.read_ldr()) and not np.array_equal(ldr, b.read_ldr()) and not np.array_equal(ldr, metered)
        # invalid input changes nothing; a later crh_set_params restarts and takes its own three values
        for bad in ((1, np.nan, 1.0), (1, 0.0, np.inf), (0, -np.inf, 1.0)):
            with pytest.raises(BackendError):
                a.set_display(*bad)
        assert a.get_display() == dict(tonemap_mode=1, exposure=1.25, white_point=3.0, auto_on=False)
        with pytest.raises(BackendError):
            a.set_auto_exposure(True, key_stops=np.nan)
        assert not a.get_display()["auto_on"]
        a.set_params(dataclasses.replace(sc.params, exposure=-0.5))
        assert a.get_display() == dict(tonemap_mode=sc.params.tonemap_mode, exposure=-0.5, white_point=float(F32(sc.params.white_point)), auto_on=False)
        assert a.save_accum()[1] == 0
    finally:
        for v in (a, b, c):
            v.close()
