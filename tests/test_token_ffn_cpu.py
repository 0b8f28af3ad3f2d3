"""The row map of the fused feed-forward kernel (csrc/token_gemm_split.hip), restated on the host.

fc1's accumulator tiles become fc2's B fragments without leaving the registers.  For v_mfma_f32_16x16x32_bf16, lane
(j, g) of a 16 x 16 fp32 C tile holds rows 4g .. 4g + 3 of column j in its registers e = 0 .. 3; a B fragment of a
32-deep k-step wants, in lane (j, g), k = 8g .. 8g + 7 of column j in its elements 0 .. 7.  Step i of fc2 takes elements
4h + e from register e of row tile 2i + h, so row position (row tile 2i + h, row 4g + e) of W1's split has to hold hidden
feature 32i + 8g + 4h + e of the slice: then the fragment is in natural k order and fc2 reads the plain split of W2."""
import pytest

from weed_instance_segmentation_amd import _lib


def ffn_row(n: int) -> int:
    """Row position n of the split -> the row of W1 it holds (include/wm2f.h, WM2F_ROWS_FFN)."""
    block, rt, r = n // 32, (n // 16) % 2, n % 16
    g, e = r // 4, r % 4
    return 32 * block + 8 * g + 4 * rt + e


def c_tile_row(g: int, e: int) -> int:
    """The row of a 16 x 16 C tile that lane group g holds in register e."""
    return 4 * g + e


def b_fragment_k(g: int, element: int) -> int:
    """The k of a 32-deep k-step that lane group g holds in element `element` of its B fragment."""
    return 8 * g + element


@pytest.mark.parametrize("F", [256, 512, 768, 1024])
def test_row_map_permutes_every_block_of_32(F):
    for block in range(F // 32):
        rows = [ffn_row(n) for n in range(32 * block, 32 * block + 32)]
        assert sorted(rows) == list(range(32 * block, 32 * block + 32))
    assert sorted(ffn_row(n) for n in range(F)) == list(range(F))


@pytest.mark.parametrize("F", [256, 1024])
def test_accumulator_registers_are_the_next_fragment_in_natural_k_order(F):
    for s in range(F // 256):
        for i in range(8):  # fc2's k-step 8s + i
            for g in range(4):
                for h in range(2):
                    for e in range(4):
                        position = 256 * s + 16 * (2 * i + h) + c_tile_row(g, e)  # where fc1 left this register's value
                        feature = ffn_row(position)
                        k = 32 * (8 * s + i) + b_fragment_k(g, 4 * h + e)  # the k fc2's A operand has in that element
                        assert feature == k, (s, i, g, h, e)


def test_bias_is_read_through_the_same_map():
    """Registers 0 .. 3 of (row tile rt, lane group g) hold four CONSECUTIVE hidden features starting at
    32 (rt // 2) + 8g + 4 (rt % 2): the kernel adds b1 as one 16-byte read at that offset."""
    for rt in range(16):
        for g in range(4):
            first = 32 * (rt // 2) + 8 * g + 4 * (rt % 2)
            assert [ffn_row(16 * rt + 4 * g + e) for e in range(4)] == [first + e for e in range(4)]


def test_library_agrees():
    lib = _lib.load()
    assert [lib.wm2f_token_ffn_row(n) for n in range(1024)] == [ffn_row(n) for n in range(1024)]
    assert lib.wm2f_token_ffn_row(-1) == -1
