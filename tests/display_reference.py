"""An OUTSIDE reference of the display and adaptive-sampling back end -- float64 numpy, written from the definitions (DESIGN.md
section 3 "Accumulator (a15), display (a17)", include/crh_spec.h #15, the prose above the kernels in
cadrays_amd/csrc/k_accumulate.h), NOT from k_accumulate.h's code or oracle/crh_oracle.c, which are transliterations of each
other.  tests/test_display_backend.py compares the oracle (CPU) and the gfx950 kernels against it, so that an error the twins
share -- a wrong filmic constant, a variance divided by the wrong count, swapped luma weights, an off-by-one in the CDF search, a
lost carry between chunks -- shows up.

Nothing here rounds to float32 on the way: every result is the exact-arithmetic value (to float64 accuracy) of the float32 inputs
it is given; what float32 arithmetic may do to it is the business of the bounds in the test module and of the ones returned below.
"""
import numpy as np

EPS = 2.0 ** -24                                          # half an ulp of 1 in float32

# ---------------------------------------------------------------------------------------------------- tone map
# John Hable's filmic curve ("Uncharted 2"): shoulder strength, linear strength, linear angle, toe strength, toe numerator, toe denominator
HABLE_A, HABLE_B, HABLE_C, HABLE_D, HABLE_E, HABLE_F = 0.22, 0.30, 0.10, 0.20, 0.01, 0.30


def filmic(x):
    """((x (A x + C B) + D E) / (x (A x + B) + D F)) - E / F for x >= 0, +inf included: above 1 numerator and denominator are divided
    through by x^2, so the value tends to its limit A / A - E / F instead of inf / inf"""
    x = np.asarray(x, np.float64)
    A, B, C, D, E, F = HABLE_A, HABLE_B, HABLE_C, HABLE_D, HABLE_E, HABLE_F
    small = x <= 1.0
    xs = np.where(small, x, 1.0)
    lo = (xs * (A * xs + C * B) + D * E) / (xs * (A * xs + B) + D * F)
    with np.errstate(divide="ignore"):
        t = 1.0 / np.where(small, 1.0, x)                  # in [0, 1): 0 for x = +inf
    hi = (A + C * B * t + D * E * t * t) / (A + B * t + D * F * t * t)
    return np.where(small, lo, hi) - E / F


def display_value(rgb, mode, exposure, white_point, gamma22):
    """the display value y^(1 / gamma) in [0, 1] (float64) of float32 accumulator values: NaN or negative -> 0; gain 2^exposure; mode 1: the
    filmic curve over its value at the white point (a white point <= 0 means 1); clamp to [0, 1]; gamma 2.2 or gamma 2.  Exposure and
    white point are taken as the float32 values the parameter block carries"""
    x = np.asarray(rgb, np.float32).astype(np.float64)
    x = np.where(np.isnan(x) | (x < 0), 0.0, x)
    x = x * 2.0 ** float(np.float32(exposure))
    if mode == 1:
        wp = float(np.float32(white_point))
        x = filmic(x) / filmic(wp if wp > 0 else 1.0)
    y = np.clip(x, 0.0, 1.0)
    return y ** (1.0 / 2.2) if gamma22 else np.sqrt(y)


def tonemap(rgb, mode, exposure, white_point, gamma22):
    """(v, byte): the unrounded v = 255 y + 0.5 in float64 and the byte floor(v)"""
    v = 255.0 * display_value(rgb, mode, exposure, white_point, gamma22) + 0.5
    return v, np.floor(v).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- variance estimate, tile error
LUMA = np.array([0.2126, 0.7152, 0.0722])                 # Rec. 709 luminance of linear RGB


def tile_rect(t, width, height, ts):
    tx = (width + ts - 1) // ts
    x0, y0 = (t % tx) * ts, (t // tx) * ts
    return slice(y0, min(y0 + ts, height)), slice(x0, min(x0 + ts, width))


def n_tiles(width, height, ts):
    return ((width + ts - 1) // ts) * ((height + ts - 1) // ts)


def tile_error_bounds(samples, counts, width, height, tile_size):
    """samples[k]: (H, W, 3) radiance of sample k; counts[t]: samples tile t has taken.  Per pixel, over the tile's first n samples:
    l = luminance, var = mean(l^2) - mean(l)^2, error = sqrt(max(var, 0) / n), or 1e3 where n < 2; tile error = mean over the tile's
    pixels inside the image.  Returns (value, lower, upper) per tile; the bounds replace var by var -+ B with
    B = 4 n 2^-24 max_k(l_k^2): the float32 running-mean recurrence m <- m + (v - m) / (k + 1) takes n steps of two roundings each
    (forward bound 2 n 2^-24 max|v| for m2 = mean(l^2) and, squared, for mean(l)^2 likewise), doubled"""
    samples = np.asarray(samples, np.float64)
    nt = n_tiles(width, height, tile_size)
    out = np.zeros((3, nt))
    lum = samples @ LUMA                                  # (K, H, W)
    for t in range(nt):
        ys, xs = tile_rect(t, width, height, tile_size)
        n = int(counts[t])
        if n < 2:
            out[:, t] = 1.0e3
            continue
        l = lum[:n, ys, xs]
        var = (l * l).mean(0) - l.mean(0) ** 2
        B = 4.0 * n * EPS * (l * l).max(0)
        for j, v in enumerate((var, var - B, var + B)):
            out[j, t] = np.sqrt(np.maximum(v, 0.0) / n).mean()
    return out[0], out[1], out[2]


# ---------------------------------------------------------------------------------------------------- the pick rule
def radical_inverse_24(i):
    """the base-2 radical inverse of the 32-bit integer i (its bits mirrored about the binary point), cut to 24 bits"""
    i = int(i) & 0xffffffff
    r = 0.0
    for b in range(24):
        if (i >> b) & 1:
            r += 2.0 ** -(b + 1)
    return r


def adaptive_picks(err, pick0, n_picks):
    """Draw k = 0 .. n_picks - 1: u = radical_inverse_24(pick0 + k), x = u S with S = sum of max(err, 0); the tile is the first one whose
    running sum (float64) exceeds x, or the last tile; with S not positive it is floor(u n_tiles).

    Returns (tiles, draws): the set of tiles drawn, and per draw a dict of
      tile       the reference's tile
      distance   |x - nearest CDF boundary| in units of n_tiles 2^-24 S, the worst-case bound of a float32 running sum
      undecided  float32 arithmetic may legitimately land on another tile: the draw lies within `radius` of a boundary, where radius is
                 the smaller of that unit and an a-posteriori bound of what the float32 running sum, total and product can be off by HERE:
                 e_i = 0 up to the first partial sum that float32 cannot hold (sums of equal 1e3's are exact, as are all before the first
                 rounding), (i - r + 1) 2^-24 s_i from that index r on; plus u e_last for the total; plus 2^-24 x where u S does not fit
                 float32.  Where everything is exact the radius is 0 and nothing is undecided, a draw exactly ON a boundary included
                 (`exceeds` decides it on both sides)
      lo, hi     the tiles such a draw may land on (lo .. hi inclusive; lo = hi = tile when decided)"""
    e = np.maximum(np.asarray(err, np.float32).astype(np.float64), 0.0)
    e = np.where(np.isnan(e), 0.0, e)
    n = len(e)
    s = np.cumsum(e)
    S = float(s[-1])
    draws, tiles = [], set()
    if not S > 0.0:
        for k in range(n_picks):
            z = radical_inverse_24(pick0 + k) * n
            t = min(int(np.floor(z)), n - 1)
            und = (np.ceil(z) - z) < n * EPS and np.ceil(z) != z and t + 1 < n     # a float32 product may round up to the next integer
            draws.append(dict(tile=t, distance=np.inf, undecided=bool(und), lo=t, hi=t + 1 if und else t))
            tiles.add(t)
        return tiles, draws
    unit = n * EPS * S
    inexact = np.flatnonzero(s.astype(np.float32).astype(np.float64) != s)
    e_cdf = np.zeros(n)
    if len(inexact):
        r = int(inexact[0])
        e_cdf[r:] = (np.arange(r, n) - r + 1) * EPS * s[r:] * (1.0 + 2.0 ** -20)
    for k in range(n_picks):
        u = radical_inverse_24(pick0 + k)
        x = u * S
        t = min(int(np.searchsorted(s, x, side="right")), n - 1)            # first s[t] > x
        e_x = 0.0 if (e_cdf[-1] == 0.0 and float(np.float32(x)) == x) else EPS * x * (1.0 + 2.0 ** -20)
        rad = np.minimum(e_cdf + u * e_cdf[-1] + e_x, unit)
        above, surely = (s + rad) > x, (s - rad) > x
        lo = int(np.argmax(above)) if above.any() else n - 1                # the first tile whose float32 sum could exceed x
        hi = int(np.argmax(surely)) if surely.any() else n - 1              # the first one whose sum must: nothing later is the first
        und = (rad > 0).any() and lo != hi
        near = np.abs(s - x).min()
        draws.append(dict(tile=t, distance=float(near / unit), undecided=bool(und), lo=lo, hi=hi))
        tiles.add(t)
    return tiles, draws
