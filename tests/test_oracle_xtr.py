"""Pins oracle/xtr_text.py (LDM BERTEmbedder's x-transformers encoder): against the committed reference output
(tests/golden/xtr_text_tiny.npz, written by oracle/gen_golden.py from the reference's own module) and, at another
size, against that module directly where the reference tree exists, else against the committed record of its run."""
import json

import torch

import golden_util as gu
from oracle import gen_golden as gg
from oracle import ref_import, xtr_text as ox


def test_oracle_matches_reference_fixture():
    fx = gu.load("xtr_text_tiny")
    cfg = ox.XtrTextCfg(width=int(fx["width"]), layers=int(fx["layers"]), vocab=int(fx["vocab"]), positions=77)
    sd = ox.synth_state_dict(cfg, int(fx["wseed"]))
    with torch.no_grad():
        y = ox.xtr_text_forward(sd, cfg, torch.as_tensor(fx["ids"]))
    assert torch.allclose(y, torch.as_tensor(fx["y"]), atol=2e-5, rtol=1e-5), (y - torch.as_tensor(fx["y"])).abs().max()


def test_oracle_matches_reference_module():
    """another width / depth / length: against the reference's module where the reference tree holds it, else against the
    committed record of that module's run (tests/golden/xtr_text_module_check.npz, oracle/gen_golden.py --only records)"""
    c = gg.XTR_CHECK
    cfg = ox.XtrTextCfg(width=c["width"], layers=c["layers"], vocab=c["vocab"], positions=c["positions"])
    ids = gg.xtr_check_ids()
    if gg.reference_has(gg.XTR_FILES):
        with ref_import.session():
            shapes, ref = gg.xtr_module_run(cfg, c["wseed"], ids)
    else:
        fx = gu.load("xtr_text_module_check")
        assert torch.equal(ids, torch.as_tensor(fx["ids"])) and int(fx["wseed"]) == c["wseed"]
        shapes, ref = {k: tuple(v) for k, v in json.loads(str(fx["shapes"])).items()}, torch.as_tensor(fx["y"])
    assert shapes == dict(ox.param_shapes(cfg))
    sd = ox.synth_state_dict(cfg, c["wseed"])
    with torch.no_grad():
        assert torch.allclose(ox.xtr_text_forward(sd, cfg, ids), ref, atol=2e-5, rtol=1e-5)
