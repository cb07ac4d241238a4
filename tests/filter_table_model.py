"""NumPy restatement of the cfconv filter table (csrc/mp_cfconv.hip: ``mp_cfconv_filter_table_layout``,
``cfconv_filter_table_kernel``, ``ft_point``, ``ft_accumulate``), written from the formulas in the kernel's comments and
DESIGN.md 3.28, without any engine import: the domain rule, the power-of-two spacing, the clamp, the six Lagrange weights
and the accumulation in fixed order, every step rounded to float32 where the kernel rounds, and the float64 filter the
table is made from."""
import numpy as np

F = 128
MAX_ROWS = 256
f32 = np.float32


def layout(bins, distance, sigma, offset, log2_inv_h=5):
    """``mp_filter_table_layout``: v = d - offset runs from max(-offset, -7 sigma) to distance (bins-1)/bins + 7 sigma,
    up to the next multiple of h = 2^-log2_inv_h; rows = intervals + 5 (nodes -2 .. 3 around every interval), padded to
    even.  ``None`` where the table does not fit."""
    distance, sigma, offset = float(f32(distance)), float(f32(sigma)), float(f32(offset))
    h = 1.0 / (1 << log2_inv_h)
    reach = 7.0 * abs(sigma)
    v_lo = f32(max(-offset, -reach))
    v_hi = distance * (bins - 1) / bins + reach
    n = int(np.ceil((v_hi - float(v_lo)) / h))
    if n < 1 or n + 6 > MAX_ROWS:
        return None
    return {"v_lo": v_lo, "v_end": f32(float(v_lo) + n * h), "inv_h": f32(1 << log2_inv_h), "n_int": n,
            "rows": (n + 5 + 1) & ~1, "h": h}


def filter64(v, w1, b1, w2, b2, distance, sigma):
    """The filter Dense(F, linear)(Dense(F, ssp)(gauss)) in float64 at v = d - offset (any shape): (..., 128)."""
    v = np.asarray(v, np.float64)
    bins = w1.shape[0]
    distance, sigma = float(f32(distance)), float(f32(sigma))
    mu = np.arange(bins, dtype=np.float64) / bins * distance
    gamma = 1.0 / sigma / sigma / 2.0
    g = np.exp(-gamma * (v[..., None] - mu) ** 2)
    pre = g @ w1.astype(np.float64)
    if b1 is not None:
        pre = pre + b1.astype(np.float64)
    hid = np.logaddexp(0.0, pre) - np.log(2.0)
    out = hid @ w2.astype(np.float64)
    return out + b2.astype(np.float64) if b2 is not None else out


def knots(L):
    return float(L["v_lo"]) + (np.arange(L["n_int"] + 5, dtype=np.float64) - 2.0) * L["h"]


def build_table(L, w1, b1, w2, b2, distance, sigma):
    """(rows, 128) float32: the float64 filter at the knots, rounded once; padding rows zero."""
    t = np.zeros((L["rows"], F), f32)
    t[:L["n_int"] + 5] = filter64(knots(L), w1, b1, w2, b2, distance, sigma).astype(f32)
    return t


def point(d, offset, L):
    """``ft_point`` in float32: (weights (n, 6), interval (n)) of distances ``d``."""
    d = np.asarray(d, f32)
    v = np.minimum(np.maximum(d - f32(offset), L["v_lo"]), L["v_end"]).astype(f32)
    t = ((v - L["v_lo"]).astype(f32) * L["inv_h"]).astype(f32)
    i = np.clip(t.astype(np.int32), 0, L["n_int"] - 1)
    u = (t - i.astype(f32)).astype(f32)
    f0, f1, f2, f3, f4, f5 = u + f32(2), u + f32(1), u, u - f32(1), u - f32(2), u - f32(3)
    a, b, c = f0 * f1, f2 * f3, f4 * f5
    bc, ac, ab = b * c, a * c, a * b
    w = np.stack([(f1 * bc) * f32(-1.0 / 120.0), (f0 * bc) * f32(1.0 / 24.0), (f3 * ac) * f32(-1.0 / 12.0),
                  (f2 * ac) * f32(1.0 / 12.0), (f5 * ab) * f32(-1.0 / 24.0), (f4 * ab) * f32(1.0 / 120.0)], axis=-1)
    assert w.dtype == f32
    return w, i


def interpolate(table, d, offset, L):
    """``ft_accumulate`` over the rows i .. i + 5 in the kernel's order: one float32 product, then five fused
    multiply-adds (the product of two float32 is exact in float64; its sum with the accumulator is rounded to float64
    and then to float32 - the double rounding differs from a true FMA in about one case in 2^29)."""
    w, i = point(d, offset, L)
    acc = (w[:, 0, None] * table[i]).astype(f32)
    for k in range(1, 6):
        acc = (w[:, k, None].astype(np.float64) * table[i + k].astype(np.float64) + acc.astype(np.float64)).astype(f32)
    return acc


def check_points(L, offset):
    """The distances of the build's self-check: quarter, half and three-quarter points of every interval and four points
    beyond the ends (the low one not below d = 0: where the domain starts at -offset nothing lies in front of it), as
    float32 distances."""
    h = f32(L["h"])
    q = np.arange(3 * L["n_int"])
    v = (L["v_lo"] + ((q // 3).astype(f32) + f32(0.25) * (q % 3 + 1).astype(f32)) * h).astype(f32)
    ends = np.array([max(L["v_lo"] - f32(1), -f32(offset)), L["v_end"] + f32(0.015625), L["v_end"] + f32(4), L["v_end"] + f32(1000)], f32)
    return (np.concatenate([v, ends]) + f32(offset)).astype(f32)


def error_over_scale(table, d, offset, L, w1, b1, w2, b2, distance, sigma):
    """(largest |interpolant - float64 filter at the float32-rounded v| over ``d``) / (largest |filter| there)."""
    d = np.asarray(d, f32)
    ref = filter64((d - f32(offset)).astype(f32), w1, b1, w2, b2, distance, sigma)
    got = interpolate(table, d, offset, L).astype(np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
