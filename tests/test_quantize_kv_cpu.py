"""bsmr.autograd.quantize_kv on CPU tensors: per-tensor amax / 448 scales into torch.float8_e4m3fn."""
import torch

from bsmr.autograd import quantize_kv


def test_grid_values_round_trip_and_amax_maps_to_448():
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[torch.isfinite(grid)].reshape(2, -1)  # every finite e4m3 value, +-448 among them
    K8, V8, ks, vs = quantize_kv(grid, -3.0 * grid)
    assert K8.dtype == V8.dtype == torch.float8_e4m3fn and ks == 1.0 and vs == 3.0
    assert torch.equal(K8.float(), grid) and torch.equal(V8.float(), -grid)
    X = torch.linspace(-0.7, 0.3, 96).reshape(4, 24)
    X8, _, s, _ = quantize_kv(X, X)
    assert s == float(torch.tensor(0.7) / 448) and X8.float().min() == -448 and X8.float().abs().max() == 448
    assert ((X8.float() * s - X).abs() <= 2.0 ** -4 * X.abs() + s * 2.0 ** -10).all()  # 3 mantissa bits, 2^-9 the least


def test_zeros_get_scale_one():
    K8, V8, ks, vs = quantize_kv(torch.zeros(3, 16), torch.ones(3, 16))
    assert ks == 1.0 and vs == float(torch.tensor(1.0) / 448) and not K8.float().any() and (V8.float() == 448).all()
