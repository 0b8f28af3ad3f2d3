"""The split of fp32 operands into three bf16 pieces that wm2f_token_linear_split_fwd accumulates (csrc/token_gemm_split.hip,
DESIGN.md §13), restated on the host: h = bf16(clamp(x)), m = bf16(x - h), l = bf16(x - h - m), round to nearest even."""
import numpy as np

BF16_MAX = np.float32(3.38953139e38)


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """Round finite fp32 to the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def split3(x: np.ndarray):
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rne(np.clip(x, -BF16_MAX, BF16_MAX))
    r1 = (x - h).astype(np.float32)
    m = bf16_rne(r1)
    r2 = (r1 - m).astype(np.float32)
    lo = bf16_rne(r2)
    return h, m, lo


def _recombined(x):
    h, m, lo = split3(x)
    return h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64)


def test_split_is_exact_on_random_fp32():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200_000), rng.standard_normal(50_000) * 1e-30,
                        rng.standard_normal(50_000) * 1e30]).astype(np.float32)
    x = np.concatenate([x, rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[np.isfinite(x) & ((np.abs(x) >= 2.0 ** -110) | (x == 0))]
    assert np.array_equal(_recombined(x), x.astype(np.float64))
    h, m, lo = split3(x)
    ax = np.abs(x.astype(np.float64))
    assert np.all(np.abs(m) <= 2.0 ** -8 * ax) and np.all(np.abs(lo) <= 2.0 ** -16 * ax)


def test_split_near_flt_max_stays_finite_and_exact():
    fmax = np.finfo(np.float32).max
    x = np.array([fmax, -fmax, np.nextafter(fmax, 0, dtype=np.float32), BF16_MAX, np.float32(3.3961e38), -np.float32(3.3961e38)],
                 dtype=np.float32)
    h, m, lo = split3(x)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(m)) and np.all(np.isfinite(lo))
    assert np.array_equal(_recombined(x), x.astype(np.float64))
    assert np.array_equal(bf16_rne(np.array([fmax], np.float32)).view(np.uint32), np.array([0x7F800000], np.uint32))  # why the clamp


def test_split_of_subnormals_loses_at_most_half_a_bf16_subnormal_step():
    rng = np.random.default_rng(1)
    bits = rng.integers(1, 1 << 23, 100_000).astype(np.uint32)  # positive fp32 subnormals
    x = np.concatenate([bits.view(np.float32), -bits.view(np.float32), (rng.standard_normal(10_000) * 2.0 ** -115).astype(np.float32)])
    err = np.abs(_recombined(x) - x.astype(np.float64))
    assert err.max() <= 2.0 ** -134


def test_six_products_are_within_2e_minus_25_of_the_exact_dot_product():
    rng = np.random.default_rng(2)
    for K, scale in ((256, 1.0), (1024, 0.05), (256, 1e-20)):
        x = (rng.standard_normal((64, K)) * scale).astype(np.float32)
        w = (rng.standard_normal((48, K)) * 0.1).astype(np.float32)
        xh, xm, xl = (p.astype(np.float64) for p in split3(x))
        wh, wm, wl = (p.astype(np.float64) for p in split3(w))
        six = xh @ wh.T + xh @ wm.T + xm @ wh.T + xh @ wl.T + xl @ wh.T + xm @ wm.T
        exact = x.astype(np.float64) @ w.astype(np.float64).T  # every fp32 product is exact in fp64, sums to 2^-53
        mag = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
        assert np.all(np.abs(six - exact) <= 2.0 ** -25 * mag)


def test_nonfinite_inputs_leave_nonfinite_pieces():
    with np.errstate(invalid="ignore"):
        h, m, lo = split3(np.array([np.inf, -np.inf, np.nan], np.float32))
    assert np.all(~np.isfinite(h + m + lo))
