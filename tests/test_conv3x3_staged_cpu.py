"""Host side of the staged route of the split 3x3 convolution (csrc/conv3x3_split.hip): the rule
wm2f_conv3x3_split_route walked over a lattice of shapes, and the halo index map of conv3x3_staged_kernel restated on the
host and compared with the direct loader's window corner + tap offset.  No GPU."""
import ctypes

import numpy as np

from weed_instance_segmentation_amd import _lib

CFG = [(16, 1), (8, 2), (4, 4), (8, 1), (4, 1)]  # (NRT, WN) of the tile table
TH, TW = 8, 32
HW_, HALO = TW + 2, (TH + 2) * (TW + 2)
LDS_LIMIT = 163840


def _staged_lds(nrt, pieces):
    return pieces * (2 * nrt * 1024 + 4 * HALO * 16)


def test_lds_budget_of_the_built_tile():
    assert HALO == 340 and _staged_lds(16, 3) == 163584 <= LDS_LIMIT
    assert _staged_lds(8, 3) == 114432 and _staged_lds(4, 3) == 89856


def test_route_lattice():
    lib = _lib.load()
    route, config = lib.wm2f_conv3x3_split_route, lib.wm2f_conv3x3_split_config
    entry = ctypes.c_int(0)
    picked = 0
    for N in (64, 128, 192, 256, 320, 512, 1024, 2048):
        for H, W in ((1, 1), (2, 3), (7, 9), (8, 32), (9, 33), (16, 16), (32, 32), (33, 31), (64, 64), (100, 75), (128, 128),
                     (256, 256)):
            for stride in (1, 2):
                for B in (1, 8):
                    for n_cu in (64, 256, 304):
                        for P in (1, 2, 3):
                            entry.value = -7
                            r = route(N, H, W, stride, B, n_cu, P, ctypes.byref(entry))
                            what = (N, H, W, stride, B, n_cu, P, r, entry.value)
                            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                            assert r in (0, 1) and 0 <= entry.value < len(CFG), what
                            assert entry.value == config(N, Ho * Wo, B, n_cu), what  # the entry is the tile rule's
                            nrt, wn = CFG[entry.value]
                            assert N % (wn * nrt * 16) == 0, what
                            if r == 1:
                                picked += 1
                                assert stride == 1 and wn == 1, what
                                assert _staged_lds(nrt, P) <= LDS_LIMIT, what
                                tiles = -(-H // TH) * -(-W // TW)
                                assert tiles <= 65535, what
                                assert H % TH == 0 and W % TW == 0, what  # whole tiles: the direct kernel's workgroups
                                per = N // (nrt * 16) * B
                                assert tiles == H * W // 256
                                assert nrt != 4 or per * tiles <= n_cu, what  # NRT 4: one round only
    assert picked > 0
    for bad in ((0, 8, 8, 1, 1, 256, 3), (96, 8, 8, 1, 1, 256, 3), (64, 0, 8, 1, 1, 256, 3), (64, 8, 8, 3, 1, 256, 3),
                (64, 8, 8, 1, 0, 256, 3), (64, 8, 8, 1, 1, 0, 3), (64, 8, 8, 1, 1, 256, 0), (64, 8, 8, 1, 1, 256, 4)):
        assert route(*bad, ctypes.byref(entry)) == -1, bad


def test_benchmark_sites():
    """The stride-1 sites of the benchmark (B = 8, 1024^2) on 256 CUs: the maps are whole tiles, so the staged kernel
    needs exactly the direct kernel's workgroups.  Stage 1 (NRT 4, eight rounds) stays on the direct kernel, the others
    measured faster staged (profiles/r15_conv3x3_staged_sites.jsonl)."""
    route = _lib.load().wm2f_conv3x3_split_route
    entry = ctypes.c_int(0)
    for N, S, want in ((64, 256, 0), (128, 128, 1), (256, 64, 1), (512, 32, 1), (256, 256, 1)):
        assert route(N, S, S, 1, 8, 256, 3, ctypes.byref(entry)) == want, (N, S)
        assert CFG[entry.value][1] == 1, (N, S, entry.value)
        assert -(-S // TH) * -(-S // TW) == S * S // 256


def test_halo_index_map_addresses_the_direct_loaders_pixels():
    """For every (tile, wave, column tile, lane, tap): the staged B read of lane (j, g) is LDS slot g * HALO + hp with
    hp = (wave + dy) * 34 + 16 c + j + dx; the staging item that filled that slot loaded pixel (h0 - 1 + hp // 34,
    w0 - 1 + hp % 34), or stored zero outside the map.  The direct loader reads the window corner (ho - 1, wo - 1) plus
    (dy, dx) where bit 3 dy + dx of tap_ok is set and zero elsewhere.  Pixel ids are 1 + h * W + w, zero for "a zero"."""
    for H, W in ((1, 1), (2, 3), (17, 1), (1, 17), (8, 32), (9, 33), (15, 31), (3, 67), (20, 70)):
        ids = 1 + np.arange(H * W).reshape(H, W)
        for ty in range(-(-H // TH)):
            for tx in range(-(-W // TW)):
                h0, w0 = ty * TH, tx * TW
                # staging: item s = g * HALO + hp, s = r * 512 + tid; slot address s * 16 per piece
                slot = np.zeros(HALO, dtype=np.int64)
                seen = np.zeros(4 * HALO, dtype=bool)
                for r in range(3):
                    for tid in range(512):
                        s = r * 512 + tid
                        if s >= 4 * HALO:
                            continue  # never written
                        seen[s] = True
                        hp = s % HALO
                        hi, wi = h0 - 1 + hp // HW_, w0 - 1 + hp % HW_
                        slot[hp] = ids[hi, wi] if 0 <= hi < H and 0 <= wi < W else 0
                assert seen.all()
                for wave in range(8):
                    for c in range(2):
                        for j in range(16):
                            ho, wo = h0 + wave, w0 + 16 * c + j
                            if ho >= H or wo >= W:
                                continue  # not stored
                            for tap in range(9):
                                dy, dx = divmod(tap, 3)
                                hp = (wave + dy) * HW_ + 16 * c + j + dx
                                assert 0 <= hp < HALO
                                hi, wi = ho - 1 + dy, wo - 1 + dx  # the direct loader: xo + tap offset under tap_ok
                                want = ids[hi, wi] if 0 <= hi < H and 0 <= wi < W else 0
                                assert slot[hp] == want, (H, W, ty, tx, wave, c, j, tap)
    # the last byte a lane reads lies inside the staged tile of every piece count
    assert (3 * HALO + (7 + 2) * HW_ + 16 + 15 + 2) * 16 + 16 <= 4 * HALO * 16
