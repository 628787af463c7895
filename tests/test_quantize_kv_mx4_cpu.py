"""CPU: the MXFP4 record format of bsmr.autograd.quantize_kv_mx4 / dequantize_mx4 (include/bsmr.h,
bsmr_attention_panels_kv4): the layout byte by byte, the round trip on grid data and the quantiser's
rules for the block exponent."""
import pytest

torch = pytest.importorskip("torch")

from bsmr import mx4_record_bytes  # noqa: E402
from bsmr.autograd import dequantize_mx4, quantize_kv_mx4  # noqa: E402

GRID = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])


def test_record_layout_byte_by_byte():
    assert (mx4_record_bytes(128), mx4_record_bytes(256)) == (80, 144)
    X = torch.zeros(1, 128)
    X[0, :4] = torch.tensor([6.0, -1.5, 0.5, -4.0])  # codes 7, 0xB, 1, 0xE: bytes 0xB7, 0xE1
    X[0, 32 + 5] = 0.75                              # block 1: 6 x 2^-3, code 7, the high nibble of byte 18
    rec, _, ks, vs = quantize_kv_mx4(X, torch.zeros(1, 256))
    want = torch.zeros(80, dtype=torch.uint8)
    want[0], want[1], want[18], want[64], want[65] = 0xB7, 0xE1, 0x70, 127, 124
    want[66:68] = 124  # blocks of zeros: floor(log2 0) is frexp's 0 - 1, so exponent -3; any would do
    assert ks == 1.0 and vs == 1.0 and rec.shape == (1, 80) and rec.dtype == torch.uint8
    assert rec[0].tolist() == want.tolist()
    assert torch.equal(dequantize_mx4(rec, 128, torch.float16), X.half())
    rec[0, 65] = 0xFF  # a NaN scale: its block, and nothing else
    assert torch.equal(dequantize_mx4(rec, 128, torch.float32).isnan()[0], torch.arange(128) // 32 == 1)


@pytest.mark.parametrize("lead", [(), (3,), (2, 3)])
def test_grid_data_survives_the_round_trip(lead):
    g = torch.Generator().manual_seed(7)
    K = GRID[torch.randint(0, 16, lead + (5, 256), generator=g)]
    K[..., 31::32] = 6.0  # pins each block's exponent
    K = K * torch.exp2(-(torch.arange(256) // 32 * 2).float())  # exponents 0, -2, .., -14: the last one is clamped
    K4, V4, ks, vs = quantize_kv_mx4(K, K[..., :128] * 0.375)  # V: amax 2.25, scale 0.375
    assert K4.shape == lead + (5, 144) and V4.shape == lead + (5, 80) and ks == 1.0 and vs == 0.375
    assert K4[..., 128:136].unique().tolist() == [115, 117, 119, 121, 123, 125, 127]  # [-12, 0]
    back = dequantize_mx4(K4, 256, torch.float32)
    assert torch.equal(back[..., :224], K[..., :224])
    # the clamped block, data at 2^-14, on the grid of exponent -12: nearest, ties to even
    assert torch.equal(back[..., 224:], (K[..., 224:] * 2.0 ** 13).round() * 2.0 ** -13)
    assert torch.equal(dequantize_mx4(V4, 128, torch.bfloat16).float() * vs, K[..., :128] * 0.375)

