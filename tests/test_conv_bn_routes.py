"""The pure decisions of the ConvBN autograd node (ops/conv.py): which backward route a layer takes (bwd_route), when
the BatchNorm backward reduction of a conv's input may ride on its data gradient (_bn_complete), whether the two-pass
forward stores the conv output (_keep_y), and the shape predicates behind them. No tensors, no GPU."""
import itertools

import pytest

from distributed_tensorflow_amd.ops import conv as OC


def pw(M, C, K, stride=1):
    """Geometry of an unpadded 1x1 conv over M output pixels."""
    return (1, M * stride, stride, C, K, 1, 1, M, 1, stride, stride, 0, 0, 1, 1)


S1 = pw(32 * 56 * 56, 64, 256)    # ResNet-50 stage-1 c3 / stride-1 projection at batch 32
S2 = pw(32 * 28 * 28, 128, 512)   # stage-2 c3
ALL = dict(link_open=True, relu_bits=True, rows_taken=True, shortcut_src=False, yc_stored=True, mask_given=False,
           need_dx=True, need_dw=True, direct_w=True, x_bf16=True)


def layer(kind, level):
    """(g, role, relu, has_res, facts) of a layer of a training ResNet-50 at a level, as its backward finds them when
    its consumer took the BN-backward rows."""
    if kind == "identity_c3":
        return S1, "res", True, True, dict(ALL, yc_stored=level < 3)
    if kind == "identity_c3_stage2":
        return S2, "res", True, True, dict(ALL)
    if kind == "proj_block_c3":  # no link; the deferred projection BN rides on it
        return S1, None, True, True, dict(ALL, link_open=False, shortcut_src=True, yc_stored=level < 4)
    if kind == "shortcut":       # c3 hands the ReLU bits over only when it folded (level >= 2)
        return S1, "proj", False, False, dict(ALL, relu_bits=level >= 2, mask_given=level >= 2)
    raise ValueError(kind)


def route(kind, level, **over):
    g, role, relu, has_res, facts = layer(kind, level)
    facts.update(over)
    role = facts.pop("role", role)
    return OC.bwd_route(g, role, relu, has_res, facts.pop("training", True), level=level, **facts)


@pytest.mark.parametrize("kind, want", [
    ("identity_c3", ["general", "pw_fused", "fold_identity", "fold_identity", "fold_identity"]),
    ("proj_block_c3", ["general", "pw_fused", "fold_proj_block", "fold_proj_block", "fold_proj_block"]),
    ("shortcut", ["general", "pw_fused", "fold_shortcut", "fold_shortcut", "fold_shortcut"]),
    ("identity_c3_stage2", ["general", "general", "fold_identity", "fold_identity", "fold_identity"]),
])
def test_routes_of_the_resnet50_layers_by_level(kind, want):
    assert [route(kind, lv) for lv in range(5)] == want
    assert {route(kind, lv, training=False) for lv in range(5)} == {"frozen"}


def test_level_comes_from_the_module_switch_when_not_given(monkeypatch):
    g, role, relu, has_res, facts = layer("identity_c3", 2)
    for lv, want in ((0, "general"), (1, "pw_fused"), (2, "fold_identity")):
        monkeypatch.setattr(OC, "_FUSED_PW_BWD", lv)
        assert OC.bwd_route(g, role, relu, has_res, True, **facts) == want
    monkeypatch.setattr(OC, "_LAZY_RES", False)
    assert OC.bwd_route(g, role, relu, has_res, True, **facts) == "pw_fused"


def test_levels_3_and_4_differ_from_2_only_through_the_stored_output():
    names = sorted(ALL)
    for g, role, relu, has_res in itertools.product((S1, S2, pw(1024, 64, 256)), (None, "acc", "res", "proj"),
                                                    (False, True), (False, True)):
        for bits in itertools.product((False, True), repeat=len(names)):
            facts = dict(zip(names, bits))
            at2 = OC.bwd_route(g, role, relu, has_res, True, level=2, **facts)
            assert OC.bwd_route(g, role, relu, has_res, True, level=3, **facts) == at2
            assert OC.bwd_route(g, role, relu, has_res, True, level=4, **facts) == at2
            assert OC.bwd_route(g, role, relu, has_res, True, level=0, **facts) == "general"
    # the stage-1 identity c3 folds with y stored or not (recomputed per tile); the stage-2 one only with y stored
    assert route("identity_c3", 2, yc_stored=False) == "fold_identity"
    assert route("identity_c3_stage2", 4, yc_stored=False) == "general"
    assert route("shortcut", 4, yc_stored=False) == "pw_fused"


KINDS = ("identity_c3", "proj_block_c3", "shortcut", "identity_c3_stage2")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_fall_throughs(kind, level):
    fused = route(kind, level)
    assert fused != "general" or (kind, level) == ("identity_c3_stage2", 1)
    # no direct weight-gradient view (or no weight / data gradient wanted): separate kernels
    assert route(kind, level, direct_w=False) == "general"
    assert route(kind, level, need_dw=False, direct_w=False) == "general"
    assert route(kind, level, need_dx=False) == "general"
    assert route(kind, level, x_bf16=False) == "general"
    # the consumer's partial rows were not taken: the reduction is not done, nothing folds
    assert route(kind, level, rows_taken=False) == ("general" if kind == "identity_c3_stage2" else "pw_fused")
    # the residual-link "acc" conv joins the parked gradient in its own data gradient: never the one-pass form
    assert route(kind, level, role="acc") in ("general", "fold_proj_block")
    assert route(kind, 1, role="acc") == "general"


@pytest.mark.parametrize("kind", ["identity_c3", "identity_c3_stage2"])
def test_identity_fold_needs_the_lazy_residual(kind, monkeypatch):
    after = "pw_fused" if kind == "identity_c3" else "general"
    assert route(kind, 4) == "fold_identity"
    assert route(kind, 4, link_open=False) == after       # no link, or the first conv's backward already ran
    assert route(kind, 4, relu_bits=False) == after
    assert route(kind, 4, role=None) == after
    assert route(kind, 4, shortcut_src=True) == ("fold_proj_block" if kind == "identity_c3" else "general")
    monkeypatch.setattr(OC, "_LAZY_RES", False)
    assert route(kind, 4) == after


def test_projection_block_folds_are_stage_1_only():
    facts = layer("proj_block_c3", 4)[4]
    assert OC.bwd_route(S2, None, True, True, True, level=4, **facts) == "general"
    assert OC.bwd_route(S1, None, False, True, True, level=4, **facts) == "pw_fused"  # no ReLU on the block output
    facts = layer("shortcut", 4)[4]
    assert OC.bwd_route(S2, "proj", False, False, True, level=4, **facts) == "general"
    assert route("shortcut", 4, mask_given=False) == "pw_fused"   # c3 did not fold: it wrote the masked gradient
    assert route("shortcut", 4, role=None) == "pw_fused"


@pytest.mark.parametrize("fn, g, want", [
    (OC.pw_bwd_ok, pw(16384, 64, 256), True),
    (OC.pw_bwd_ok, pw(16383, 64, 256), False),
    (OC.pw_bwd_ok, pw(4194303, 64, 256), True),
    (OC.pw_bwd_ok, pw(4194304, 64, 256), False),      # 2 GiB bound
    (OC.pw_bwd_bn_ok, pw(4096, 128, 512), True),
    (OC.pw_bwd_bn_ok, pw(4095, 128, 512), False),
    (OC.pw_bwd_bn_ok, pw(2097151, 128, 512), True),
    (OC.pw_bwd_bn_ok, pw(2097152, 128, 512), False),
    (OC.pw_bwd_bn_ok, pw(65536, 256, 1024), False),
    (OC.pw_bwd_bn_ok, pw(16384, 64, 256, stride=2), False),
    (OC._two_pass_ok, pw(1024, 64, 256), True),
    (OC._two_pass_ok, pw(1023, 64, 256), False),
    (OC._two_pass_ok, pw(512, 128, 512), True),
    (OC._two_pass_ok, pw(511, 128, 512), False),
    (OC._two_pass_ok, pw(4096, 256, 768), False),
    (OC._two_pass_ok, pw(4096, 512, 2048), False),
])
def test_shape_predicates(fn, g, want):
    assert fn(g) is want


def test_keep_y():
    def keep(level, g=S1, relu=True, has_res=True, res_deferred=False, link_given=True, role="res", needs_grad=True):
        return OC._keep_y(g, relu, has_res, res_deferred, link_given, role, needs_grad, level=level)

    proj_block = dict(res_deferred=True, link_given=False, role=None)
    assert [keep(lv) for lv in range(5)] == [True, True, True, False, False]              # identity block's c3
    assert [keep(lv, **proj_block) for lv in range(5)] == [True, True, True, True, False]  # projection block's c3
    for lv in (3, 4):
        assert keep(lv, g=pw(16384, 64, 256)) is False
        assert keep(lv, g=pw(16383, 64, 256))
        assert keep(lv, g=S2) and keep(lv, g=pw(32 * 56 * 56, 64, 512))
        assert keep(lv, relu=False) and keep(lv, has_res=False) and keep(lv, needs_grad=False)
        assert keep(lv, link_given=False) and keep(lv, role=None) and keep(lv, role="acc")
    assert keep(4, **dict(proj_block, needs_grad=False)) and keep(4, g=S2, **proj_block)


def test_keep_y_level_comes_from_the_module_switch(monkeypatch):
    monkeypatch.setattr(OC, "_FUSED_PW_BWD", 2)
    assert OC._keep_y(S1, True, True, False, True, "res", True)
    monkeypatch.setattr(OC, "_FUSED_PW_BWD", 3)
    assert not OC._keep_y(S1, True, True, False, True, "res", True)


def test_bn_complete_variants():
    # the only consumer
    for role in (None, "res", "acc"):
        assert OC._bn_complete(1, role)
        assert not OC._bn_complete(2, role) and not OC._bn_complete(0, role)
    # ... and not a projection, whose gradient is joined with the first conv's
    assert not OC._bn_complete(1, "proj") and not OC._bn_complete(2, "proj", acc_taken=True)
    # ... or the "acc" conv that took the other consumer's parked gradient
    assert OC._bn_complete(2, "acc", acc_taken=True)
    assert OC._bn_complete(1, "acc", acc_taken=True)
    assert not OC._bn_complete(2, "acc", acc_taken=False)
    assert not OC._bn_complete(3, "acc", acc_taken=True)
    assert not OC._bn_complete(2, "res", acc_taken=True) and not OC._bn_complete(2, None, acc_taken=True)
