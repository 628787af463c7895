"""The 16 x 16 block mask of the panel attention tests (test_attention_panels_cpu.py,
test_gpu_attention_panels.py). No GPU here."""
import numpy as np


def block_mask(nb=6, per_row=4):
    """nb x nb blocks of 16 x 16, block row b holding blocks b, b + 1, ... (mod nb)."""
    cols = [np.sort(np.concatenate([16 * ((b + k) % nb) + np.arange(16) for k in range(per_row)])) for b in range(nb)]
    ci = np.concatenate([cols[r // 16] for r in range(16 * nb)]).astype(np.uint32)
    rp = (np.arange(16 * nb + 1) * 16 * per_row).astype(np.uint32)
    return 16 * nb, 16 * nb, rp, ci
