"""GPU: pc_tail6_scatter against an index-by-index numpy copy.

dcols[n][it][ih][iw][slot] = dout[n][2 it - 2 + k_t][2 ih - 2 + k_h][2 iw - 2 + k_w] where that output exists, else 0, with
slot = (k_t * 5 + k_h) * 5 + k_w < 125; slots 125 - 127 are zero.  The kernel stages the outputs a run of 28 adjacent iw can touch and
streams the rows from there, so the widths lie below one run, across two and well above, odd ones included.  A copy has one result:
np.array_equal.  The image is prefilled with a canary, the word behind it must keep it, and every case runs twice to equal bits."""
import numpy as np
import pytest
import torch

from picons_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -777.25
SP, NSLOT = 128, 125


def _ref_scatter(dout, N, I):
    It, Ih, Iw = I
    ref = np.zeros((N, It, Ih, Iw, SP), dtype=np.float32)
    for it in range(It):
        for ih in range(Ih):
            for iw in range(Iw):
                for slot in range(NSLOT):
                    o = (2 * it - 2 + slot // 25, 2 * ih - 2 + (slot // 5) % 5, 2 * iw - 2 + slot % 5)
                    if 0 <= o[0] < 2 * It and 0 <= o[1] < 2 * Ih and 0 <= o[2] < 2 * Iw:
                        ref[:, it, ih, iw, slot] = dout[:, o[0], o[1], o[2]]
    return ref


@pytest.mark.parametrize("I", [(1, 1, 1), (2, 3, 5), (1, 4, 33), (3, 2, 70)], ids=lambda I: "%dx%dx%d" % I)
def test_tail6_scatter_copy(I):
    N = 2
    g = torch.Generator().manual_seed(41)
    dout = torch.randn(N, *[2 * v for v in I], generator=g)
    ref = _ref_scatter(dout.numpy(), N, I)
    doutg = dout.to(DEV)
    words = N * I[0] * I[1] * I[2] * SP
    runs = []
    for _ in range(2):
        buf = torch.full((words + 1,), CANARY, device=DEV)
        ops.tail6_scatter(doutg, N, *I, buf)
        runs.append(buf.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    got = runs[0][:words].reshape(N, *I, SP)
    assert np.array_equal(got, ref), "dcols is not the copy of dout"
    assert (got[..., NSLOT:] == 0).all(), "slots 125 - 127 must be zero"
    assert runs[0][words] == CANARY, "the word behind the image was written"
    assert torch.equal(doutg.cpu(), dout), "dout was written"
