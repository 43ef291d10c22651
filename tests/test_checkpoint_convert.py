"""HAIS / spconv-1 checkpoint conversion (softgroup_amd.util.checkpoint, tools/convert_checkpoint.py)
against what the reference's own script wrote for the same file (tests/golden/ckpt_convert_ref.json,
recorded by tests/golden/make_ckpt_convert.py), and as a round trip: SoftGroup weights written the
spconv-1 way load back bit-identical."""
import json
import os
import sys

import torch

from softgroup_amd import synthetic
from softgroup_amd.model import SoftGroup
from softgroup_amd.util.checkpoint import convert_checkpoint_file, convert_spconv1_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_ckpt_convert as G  # noqa: E402  (checkpoint recipe; does not need the reference to import)


def test_round_trip_loads_strictly():
    torch.manual_seed(0)
    model = SoftGroup(**synthetic.SCANNET_MODEL_CFG)
    sd = model.state_dict()
    old = G.spconv1_style(sd)
    assert any('intra_ins_unet' in k for k in old) and 'score_linear.weight' in old
    new = convert_spconv1_state_dict(old)
    assert list(new) == list(sd)
    assert all(torch.equal(new[k], sd[k]) for k in sd)
    other = SoftGroup(**synthetic.SCANNET_MODEL_CFG)
    missing, unexpected = other.load_state_dict(new, strict=True)
    assert not missing and not unexpected


def test_same_file_as_the_reference_script(tmp_path):
    """the converted file equals, tensor for tensor and in key order, the reference script's output"""
    ref = json.load(open(G.OUT))
    b = tmp_path / 'b.pth'
    torch.save(G.spconv1_checkpoint(), b)
    got = torch.load(convert_checkpoint_file(str(b)))
    assert got['epoch'] == ref['epoch'] == 7 and list(got['net']) == list(ref['tensors'])
    assert G.tensor_record(got['net']) == ref['tensors']
