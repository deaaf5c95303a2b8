"""CPU: block_type "fastformer" builds with the reference's module tree (state-dict schema, tied logit projections, initialisers),
loads reference-keyed weights, its C-ABI entry points are declared and bound, and the block types without a plugin still raise."""
import json
import os

import pytest
import torch

import ctts_amd
from ctts_amd import _lib
from ctts_amd.configs import get_configs
from tests.util import schema, closed_form_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(block="fastformer"):
    pre, mc, tc = get_configs()
    mc["block_type"] = block
    return ctts_amd.CompTransTTS(pre, mc, tc)


def tied_from_layer0(sd):
    """the fixture generator's rule (tests/golden/make_goldens_fastformer.py): every layer's key of a tied logit projection carries
    layer 0's value"""
    out = dict(sd)
    for k in sd:
        parts = k.split(".")
        if len(parts) == 8 and parts[1:3] == ["layer_stack", "layers"] and parts[4:6] == ["0", "fn"] and parts[6] in (
                "to_q_attn_logits", "to_k_attn_logits"):
            out[k] = sd[".".join(parts[:3] + ["0"] + parts[4:])]
    return out


def test_fastformer_builds_with_reference_state_dict_schema():
    m = _build()
    sd, sch = m.state_dict(), schema("LJSpeech", "fastformer")
    assert list(sd) == list(sch)                      # same keys in the same order
    params = dict(m.named_parameters())
    for k, (shape, dtype, is_param) in sch.items():
        assert list(sd[k].shape) == shape, k
        assert str(sd[k].dtype) == "torch." + dtype, k
        assert (k in params) == is_param, k
    assert len(sd) == 265 and len(list(m.parameters())) == 216
    assert list(sd["decoder.layer_stack.layers.0.1.fn.w_2.weight"].shape) == [256, 1024, 1]
    assert m.encoder.d_model == 256 and m.decoder.d_model == 256


def test_logit_projections_are_tied_per_stack():
    m = _build()
    for stack in (m.encoder, m.decoder):
        layers = stack.layer_stack.layers
        for name in ("to_q_attn_logits", "to_k_attn_logits"):
            first = getattr(layers[0][0].fn, name)
            assert all(getattr(l[0].fn, name) is first for l in layers), name
            assert list(first.weight.shape) == [128, 256]      # heads and head size swapped (FastAttention(d_model, d_head, n_head))
    assert m.encoder.layer_stack.layers[0][0].fn.to_q_attn_logits is not m.decoder.layer_stack.layers[0][0].fn.to_q_attn_logits
    names = [n for n, _ in m.named_parameters() if "attn_logits" in n]
    assert names == [f"{s}.layer_stack.layers.0.0.fn.to_{q}_attn_logits.{w}" for s in ("encoder", "decoder") for q in "qk"
                     for w in ("weight", "bias")]


def test_reference_keyed_state_dict_loads():
    m = _build()
    sd = tied_from_layer0(closed_form_sd("LJSpeech", "fastformer"))
    m.load_state_dict(sd)
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v.to(got[k].dtype)), k


def test_fastformer_initialisers_follow_the_reference():
    torch.manual_seed(0)
    m = _build()
    a = m.decoder.layer_stack.layers[2][0].fn
    for lin in (a.query, a.key, a.transform, a.to_q_attn_logits, a.to_k_attn_logits):
        assert abs(float(lin.weight.std()) - 0.02) < 0.003
        assert float(lin.bias.abs().max()) == 0.0
    assert float(m.encoder.src_word_emb.weight[0].abs().max()) == 0.0
    assert abs(float(m.encoder.src_word_emb.weight[1:].std()) - 1.0) < 0.05
    w1 = m.encoder.layer_stack.layers[0][1].fn.w_1.weight
    assert float(w1.abs().max()) <= 1 / (256 * 9) ** 0.5 + 1e-7       # kaiming_uniform(a=sqrt(5)) bound = 1/sqrt(fan_in)
    ln = m.encoder.layer_stack.layers[0][0].norm
    assert torch.equal(ln.weight, torch.ones(256)) and torch.equal(ln.bias, torch.zeros(256))


@pytest.mark.parametrize("block", ["reformer", "transformer", "lstransformer", "nope"])
def test_other_block_types_still_raise(block):
    with pytest.raises(NotImplementedError):
        _build(block)


def test_stage_plan_covers_the_nested_fastformer_stack():
    from ctts_amd.dp import stage_plan
    m = _build()
    cuts, stage_of = stage_plan(m, 3)
    assert cuts == ["decoder.layer_stack.4", "decoder.layer_stack.2", "decoder.in"]
    assert stage_of("decoder.layer_stack.layers.5.1.fn.w_2.bias") == 0
    assert stage_of("decoder.layer_stack.layers.3.0.fn.query.weight") == 1
    # the tied projections are named under layer 0: their bucket closes after the stage of layer 0's backward, the last to add to them
    assert stage_of("decoder.layer_stack.layers.0.0.fn.to_q_attn_logits.weight") == 2
    assert stage_of("encoder.layer_stack.layers.0.0.fn.to_q_attn_logits.weight") == 3


def test_fastformer_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ctts.h")).read()
    for name in ("ctts_fastformer_workspace_floats", "ctts_fastformer_pool_fwd", "ctts_fastformer_pool_bwd", "ctts_fastformer_bcast",
                 "ctts_fastformer_bcast_bwd", "ctts_fastformer_resdrop"):
        assert name + "(" in hdr and name in _lib.EXPORTED_SYMBOLS, name


def test_fastformer_forward_refuses_cpu_tensors():
    from ctts_amd.synthetic import make_batch, as_model_args
    m = _build()
    with pytest.raises(Exception):
        m(*as_model_args(make_batch([8, 5], 4)))


def test_schema_fixture_counts():
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_schema_LJSpeech_fastformer.json")) as f:
        sch = json.load(f)
    assert len(sch) == 265 and sum(v[2] for v in sch.values()) == 216
