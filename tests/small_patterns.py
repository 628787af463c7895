"""The smallest legal plans (bsmr_plan_create needs nnz >= 2), shared by test_gpu_sddmm_edges.py and
test_gpu_spmm_edges.py: M or N of 1 or 2, M around one 16-row panel, a single full row, a 17 x 17
full mask."""
import numpy as np


def _csr(M, N, mask):
    mask = np.asarray(mask, bool).reshape(M, N)
    rp = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint32)
    return M, N, rp, np.nonzero(mask)[1].astype(np.uint32)


def _ragged(M, N=5):
    """Rows of 0 .. N entries (every other row empty), and one in the last row's last column."""
    r = np.arange(M)[:, None]
    c = np.arange(N)[None, :]
    return _csr(M, N, (c < (r * 3) % (N + 1)) | ((r == M - 1) & (c == N - 1)))


SMALL = {
    "1x2": _csr(1, 2, [[1, 1]]),
    "2x1": _csr(2, 1, [[1], [1]]),
    "15x5": _ragged(15),
    "16x5": _ragged(16),
    "17x5": _ragged(17),
    "row130": _csr(1, 130, np.ones((1, 130))),
    "full17": _csr(17, 17, np.ones((17, 17))),
}
