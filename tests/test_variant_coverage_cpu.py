"""CPU: the table of kernel-variant classes (tests/variant_cases.py) is COMPLETE for the training step at the product shape, every
entry is filed under the class the library reports for it, and no entry is dead.

The classes come from the library's own host-only reporters (pc_conv_variant / pc_wino_variant / pc_wgrad_variant), which run the
decision code of the launches themselves -- nothing here re-derives a dispatch heuristic.  A change to one (choose_tile, the LDS-DMA ring
depth, pc_x6_tile, the tail split, the Winograd block shapes, the weight-gradient routes) that makes a step of some m = 2..8 select a
variant the GPU parity module (tests/test_variants_gpu.py) does not run fails here, on a machine without a GPU, and names the launch."""
import pytest

from picons_amd import capi
from tests import variant_cases as V


@pytest.fixture(scope="module")
def seen():
    return V.walk()


def test_plans_hold_no_grouped_weight_gradient_op_the_walk_would_have_to_open(seen):
    """The default plans emit every weight gradient as its own launch; plan_launches opens OP_WGRAD_MULTI job lists too, should a switch bring
    them back.  Every plan has matrix launches of all three kinds."""
    kinds = {c[0] for c in seen}
    assert kinds == {"conv", "wino", "wgrad"} and capi.lib().pc_version() >= 103
    assert len({s for e in seen.values() for s in e["sizes"]}) == len(V.SIZES) * len(V.DATASETS)


def test_every_class_a_step_of_2_to_8_clips_selects_is_in_the_table(seen):
    table = {tuple(c["cls"]) for c in V.CASES}
    missing = []
    for cls in sorted(seen, key=repr):
        if cls not in table:
            b = seen[cls]["best"][1]
            missing.append("class %r\n    at sizes %s\n    e.g. %s launch of the %s list, n = %d (%s): desc = %r, ws = %d" %
                           (cls, sorted(seen[cls]["sizes"]), b["kind"], b["list"], b["n"], b["dataset"], b["desc"], b["ws"]))
    assert not missing, "%d kernel-variant classes of the product step have no case in tests/variant_cases_table.py (regenerate it: " \
                        "python -m tests.variant_cases):\n%s" % (len(missing), "\n".join(missing))


def test_every_table_entry_yields_the_class_it_is_filed_under():
    assert len(V.CASES) >= 60 and len({c["name"] for c in V.CASES}) == len(V.CASES)
    assert len({tuple(c["cls"]) for c in V.CASES}) == len(V.CASES), "two entries for one class"
    for c in V.CASES:
        got = V.case_class(c)
        assert got == tuple(c["cls"]), "%s: filed under %r, the library reports %r" % (c["name"], c["cls"], got)


def test_no_table_entry_is_dead(seen):
    dead = [c["name"] + ": " + repr(c["cls"]) for c in V.CASES if tuple(c["cls"]) not in seen]
    assert not dead, "no plan for n = 2..8 selects these classes any more (drop them from the table):\n" + "\n".join(dead)
    for c in V.CASES:
        sizes = ",".join("%s%d" % (ds[0], n) for ds, n in sorted(seen[tuple(c["cls"])]["sizes"]))
        assert sizes == c["sizes"], "%s: occurs at %s, the table says %s" % (c["name"], sizes, c["sizes"])


def test_float64_references_of_the_gpu_module_agree_with_the_descriptor_interpreter():
    """tests/test_variants_gpu.py turns a descriptor into ONE torch conv3d call (stride, dilation, padding, gathered weight taps, mirrored
    gathers walked from the other end).  On small problems that must be the sum tests/desc_interp.py spells out position by position --
    forward with stride and trimmed taps, the parity classes of an input gradient (mirrored taps, strided output lattice), and the weight
    gradient with trimmed taps."""
    import numpy as np
    import torch
    from picons_amd import desc as D
    from tests import desc_interp, test_variants_gpu as T
    g = torch.Generator().manual_seed(5)
    N, Ci, Co, thw, k, s, pf, othw = 2, 8, 12, (3, 6, 5), (3, 3, 3), (2, 1, 1), (1, 1, 1), (2, 6, 5)
    x, w = torch.randn(N, *thw, Ci, generator=g), torch.randn(1, Co, 27, Ci, generator=g)
    b, cs = torch.randn(1, Co, generator=g), torch.rand(N, Co, generator=g)
    fwd = dict(D.trim_conv(D.conv_fwd(N, thw, Ci, Ci, Co, Co, k, s, pf, othw, act=capi.ACT_RELU, flags=capi.F_BIAS | capi.F_CSCALE | capi.F_ACCUM)), act_c0=4)
    base = torch.randn(N, *othw, Co, generator=g)
    want = desc_interp.run_conv(dict(fwd, act=0), x.double().numpy(), w[0].double().numpy(), b[0].double().numpy(), cs.double().numpy(), np.zeros((N, *othw, Co)))
    got, _, _ = T.conv_reference(dict(fwd, act=0, flags=fwd["flags"] & ~capi.F_ACCUM), x, w, b, cs, torch.zeros(N, *othw, Co))
    assert np.abs(got.numpy() - want).max() < 1e-12
    got, _, _ = T.conv_reference(fwd, x, w, b, cs, base)
    pre = torch.from_numpy(desc_interp.run_conv(dict(fwd, act=0, flags=capi.F_BIAS), x.double().numpy(), w[0].double().numpy(), b[0].double().numpy(), None, np.zeros((N, *othw, Co))))
    pre = torch.cat([pre[..., :4], pre[..., 4:].clamp_min(0)], -1) * cs.double().view(N, 1, 1, 1, Co)
    assert (got - (base.double() + pre)).abs().max().item() < 1e-12
    dy, wt = torch.randn(N, *othw, Co, generator=g), torch.randn(1, Ci, 27, Co, generator=g)
    classes = D.transposed_classes(N, othw, Co, Co, thw, Ci, Ci, k, s, pf, ldw=Co)
    assert any(min(c["istep"]) < 0 for c in classes) and len(classes) >= 2
    want = np.zeros((N, *thw, Ci))
    got = torch.zeros(N, *thw, Ci, dtype=torch.float64)
    for c in classes:
        desc_interp.run_conv(c, dy.double().numpy(), wt[0].double().numpy(), out=want)
        got, _, _ = T.conv_reference(c, dy, wt, None, None, got)
    assert np.abs(got.numpy() - want).max() < 1e-12 and np.abs(want).max() > 1
    wd = D.trim_wgrad(D.wgrad(N, (2, 6, 5), Co, Co, (1, 6, 5), Ci, Ci, k, (1, 1, 1), pf))
    assert wd["ntap"][0] < 3
    Dl, S = torch.randn(N, 2, 6, 5, Co, generator=g), torch.randn(N, 1, 6, 5, Ci, generator=g)
    assert np.abs(T.wgrad_reference(wd, Dl, S).numpy() - desc_interp.run_wgrad(wd, Dl.double().numpy(), S.double().numpy())).max() < 1e-12
