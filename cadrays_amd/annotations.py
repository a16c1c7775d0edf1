"""Pure list builders for the annotations of the display (View.SetAnnotations; include/cadrays_hip.h section "annotations").

Every helper an application draws over the path-traced frame reduces to coloured world-space segments: the manipulator at the selection's pivot (ImGuizmo::Manipulate,
reference src/ImGui/ImRaytraceControls.cxx:64), a marker at every positional light (DrawLights, :93-111), and what any CAD viewer adds around those -- a ground grid,
an axis triad, the selection's box.  The builders return numpy record arrays of abi.ANNOT_SEGMENT_DTYPE (32 B per segment); join() concatenates them.  No device,
no library: plain float64 arithmetic, rounded once to the float32 fields.
"""
import math

import numpy as np

from . import abi

DTYPE = np.dtype(abi.ANNOT_SEGMENT_DTYPE)


def segments(a, b, rgb=(255, 255, 255), alpha=255, width=1, mode=abi.ANNOT_ON_TOP):
    """n segments from end points a, b ((n, 3) each, or one point of 3): one colour, alpha, width (1..8 pixels) and mode for all"""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    assert a.shape == b.shape, (a.shape, b.shape)
    out = np.zeros(len(a), DTYPE)
    out["a"], out["b"] = a, b
    out["rgb"], out["alpha"], out["style"] = np.asarray(rgb, np.uint8), int(alpha), abi.annot_style(width, mode)
    return out


def join(*lists):
    """one list of several, in the order given (later segments are drawn over earlier ones)"""
    return np.concatenate([np.asarray(l, DTYPE).reshape(-1) for l in lists]) if lists else np.zeros(0, DTYPE)


def polyline(points, closed=False, **style):
    """the segments between consecutive points ((n, 3)); closed: and from the last back to the first"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    q = np.roll(p, -1, axis=0)
    return segments(p, q, **style) if closed else segments(p[:-1], q[:-1], **style)


def grid(origin, u, v, step, count, rgb=(128, 128, 128), alpha=160, width=1, mode=abi.ANNOT_HIDE):
    """a ground grid in the plane through origin spanned by u and v: 2 count + 1 lines along u and as many along v, `step` apart, each 2 count step long
    (count = 20: the 41-line grid)"""
    o, u, v = (np.asarray(x, np.float64) for x in (origin, u, v))
    k = np.arange(-int(count), int(count) + 1, dtype=np.float64)[:, None] * float(step)
    reach = float(count) * float(step)
    along_u = segments(o + k * v - reach * u, o + k * v + reach * u, rgb, alpha, width, mode)
    along_v = segments(o + k * u - reach * v, o + k * u + reach * v, rgb, alpha, width, mode)
    return join(along_u, along_v)


def axes(origin, size, alpha=255, width=2, mode=abi.ANNOT_ON_TOP):
    """the axis triad: x red, y green, z blue, each from origin to origin + size e"""
    o = np.asarray(origin, np.float64)
    return join(*[segments(o, o + float(size) * np.eye(3)[k], tuple(255 if j == k else 0 for j in range(3)), alpha, width, mode) for k in range(3)])


def box(lo, hi, rgb=(255, 255, 0), alpha=255, width=1, mode=abi.ANNOT_XRAY):
    """the 12 edges of the axis-aligned box [lo, hi]: four along x, four along y, four along z"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])      # corner i: bit k chooses hi on axis k
    pairs = [(i, i | (1 << k)) for k in range(3) for i in range(8) if not i & (1 << k)]
    return segments(c[[p[0] for p in pairs]], c[[p[1] for p in pairs]], rgb, alpha, width, mode)


def _frame(normal):
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    t = np.eye(3)[int(np.argmin(np.abs(n)))]
    e0 = np.cross(n, t); e0 /= np.linalg.norm(e0)
    return e0, np.cross(n, e0)


def circle(centre, normal, radius, n=32, rgb=(255, 255, 255), alpha=255, width=1, mode=abi.ANNOT_ON_TOP):
    """a closed polygon of n segments on the circle around centre in the plane with this normal"""
    e0, e1 = _frame(normal)
    a = 2.0 * math.pi * np.arange(int(n), dtype=np.float64)[:, None] / float(n)
    return polyline(np.asarray(centre, np.float64) + float(radius) * (np.cos(a) * e0 + np.sin(a) * e1), closed=True, rgb=rgb, alpha=alpha, width=width, mode=mode)


def arrow(tail, head, barb=0.2, **style):
    """a shaft from tail to head and four barbs back from the head, each `barb` of the shaft's length: 5 segments"""
    tail, head = np.asarray(tail, np.float64), np.asarray(head, np.float64)
    d = head - tail
    e0, e1 = _frame(d)
    l = float(np.linalg.norm(d)) * float(barb)
    back = head - d * float(barb)
    tips = np.array([back + l * 0.5 * e0, back - l * 0.5 * e0, back + l * 0.5 * e1, back - l * 0.5 * e1])
    return join(segments(tail, head, **style), segments(np.tile(head, (4, 1)), tips, **style))


def light_markers(lights, size, anchor=(0.0, 0.0, 0.0), n=16, rgb=(255, 255, 128), alpha=255, width=1, mode=abi.ANNOT_XRAY):
    """DrawLights (ImRaytraceControls.cxx:93-111): three circles of radius `size` around every positional light (scenes.Light, is_point), one per coordinate plane;
    an arrow of length 4 size per directional one, pointing along the light's travel at `anchor`"""
    out = []
    for l in lights:
        v = np.asarray(l.vec, np.float64)
        if l.is_point:
            out += [circle(v, np.eye(3)[k], size, n, rgb, alpha, width, mode) for k in range(3)]
        else:
            to_light = v / np.linalg.norm(v)
            a = np.asarray(anchor, np.float64)
            out.append(arrow(a + 4.0 * float(size) * to_light, a, rgb=rgb, alpha=alpha, width=width, mode=mode))
    return join(*out)


MANIPULATOR_HANDLES = ("move_x", "move_y", "move_z", "turn_x", "turn_y", "turn_z")


def manipulator(pivot, size, n=32, alpha=255, width=2, mode=abi.ANNOT_ON_TOP):
    """the manipulator at the pivot (ImGuizmo::Manipulate, ImRaytraceControls.cxx:64): an arrow along each axis (5 segments each: move_x, move_y, move_z) and a circle
    of n segments around each (turn_x, turn_y, turn_z), x red, y green, z blue.  manipulator_handle(index, n) names the handle of a segment index, which is what
    View.PickAnnotation reports under the cursor."""
    o = np.asarray(pivot, np.float64)
    col = lambda k: tuple(255 if j == k else 0 for j in range(3))
    arrows = [arrow(o, o + float(size) * np.eye(3)[k], rgb=col(k), alpha=alpha, width=width, mode=mode) for k in range(3)]
    rings = [circle(o, np.eye(3)[k], 0.75 * float(size), n, col(k), alpha, width, mode) for k in range(3)]
    return join(*arrows, *rings)


def manipulator_handle(index, n=32, first=0):
    """the name of the manipulator handle segment `index` belongs to (the manipulator's segments start at `first` in the list), or None"""
    k = int(index) - int(first)
    if 0 <= k < 15:
        return MANIPULATOR_HANDLES[k // 5]
    if 15 <= k < 15 + 3 * int(n):
        return MANIPULATOR_HANDLES[3 + (k - 15) // int(n)]
    return None
