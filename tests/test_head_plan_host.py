"""Host: the structure of `modules.HeadLevelPlan`, the record by which v10Detect3d stacks the 16 branches of a head level, for each of
its three layouts (uniform widths, cls wider than the regression branches, no second-layer stack).  Built on the CPU: no kernel runs."""
import pytest
import torch

from yolov10_3d_amd import modules as M

NAMES = ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")
LAYOUTS = {  # widths per branch -> the groups of the second-layer parts
    "uniform": (dict.fromkeys(NAMES, 16), (16,)),
    "wide_cls_128_64": ({**dict.fromkeys(NAMES, 64), "cls": 128}, (1, 14, 1)),
    "wide_cls_32_16": ({**dict.fromkeys(NAMES, 16), "cls": 32}, (1, 14, 1)),
    "no_stack": ({**dict.fromkeys(NAMES, 16), "hd": 32}, ()),
}


@pytest.fixture(scope="module", params=list(LAYOUTS))
def head(request):
    widths, groups = LAYOUTS[request.param]
    torch.manual_seed(3)
    hd = M.v10Detect3d(3, (32, 64), False, {k + "_c": c for k, c in widths.items()}, False, False, False, False, 2, False, False, 3, 3)
    return hd, [widths[k] for k in NAMES] * 2, groups


def test_plan_structure(head):
    hd, canon_widths, groups = head
    for i in range(hd.nl):
        plan = hd._stacks(i)
        assert plan is hd._stacks(i), "the plan of a level is cached"
        assert sorted(plan.pos) == list(range(16))
        canon = [h[i] for h in hd.o2o_heads] + [h[i] for h in hd.o2m_heads]
        for c in range(16):
            assert plan.branches[plan.pos[c]] is canon[c] and plan.mids[plan.pos[c]] == canon_widths[c]
        assert list(plan.offs) == [sum(plan.mids[:j]) for j in range(16)]
        # the one-to-one half (its input is detached) comes first; the one-to-many half is the data-gradient window of layer 1
        assert {id(b) for b in plan.branches[:8]} == {id(b) for b in canon[:8]}
        assert plan.o2m_range == (sum(plan.mids[:8]), sum(plan.mids))
        assert [b[0] for b in plan.branches] == plan.s1.convs
        # the parts tile z1's channels and the branches, each with one group per branch
        assert tuple(p.groups for p in plan.layer2) == groups and plan.uniform == (groups == (16,))
        lo = first = 0
        for p in plan.layer2:
            assert (p.lo, p.first) == (lo, first) and p.groups * p.width == p.hi - p.lo
            brs = plan.branches[p.branches]
            assert len(brs) == p.groups and [b[1] for b in brs] == p.stack.convs and p.stack.groups == p.groups
            assert all(m == p.width for m in plan.mids[p.branches])
            lo, first = p.hi, first + p.groups
        if groups:
            assert (lo, first) == (sum(plan.mids), 16)
        assert list(plan.stacks()) == [plan.s1] + [p.stack for p in plan.layer2]
        for (off, width), set_ in zip(plan.emb, (hd.o2o_heads, hd.o2m_heads)):
            j = plan.branches.index(set_[6][i])
            assert (off, width) == (plan.offs[j], plan.mids[j])


def test_restack_shares_storage_with_the_branches(head):
    hd = head[0]
    hd.restack()
    for i in range(hd.nl):
        plan = hd._stacks(i)
        w = plan.s1.tensors()[0]
        assert w.shape[0] == sum(plan.mids)
        for b, off, mid in zip(plan.branches, plan.offs, plan.mids):
            bw = b[0].conv.weight
            assert bw.data_ptr() == w[off].data_ptr() and torch.equal(bw.detach(), w[off:off + mid])
        for p in plan.layer2:
            w2 = p.stack.tensors()[0]
            for k, b in enumerate(plan.branches[p.branches]):
                assert b[1].conv.weight.data_ptr() == w2[k * p.width].data_ptr()
