"""translate()'s host code, pinned by the sequence of engine calls it makes (no GPU): tests/_translate_calls.py drives the
wrapper on a recording stand-in engine over a grid of ensemble shapes, features (keep-mask of either source, cross-attention
control, the estimated mask) and limits (COUPLE_MAX_TOKENS, MAX_FOLD, a short white-box prefix, couple = False), and the
records - every argument's name, shape and digest, the order of the noise draws, the result, last_translate_coupled - are
held against tests/golden/translate_calls.json, recorded before the three copies of the coupled loop became one."""
import json

import pytest

import _translate_calls as tc

PRECONDITIONS = (
    "ValueError: cross-attention control needs the DPM-Encoder over the whole chain",
    "ValueError: cross-attention control: every decoder scale must ride in the coupled loop",
    "ValueError: mask_source = 'encoder' needs the DPM-Encoder over the whole chain",
    "ValueError: mask_source = 'encoder': every decoder scale must ride in the coupled loop",
    "ValueError: mask must be [3, 1, 4, 4], got (3, 1, 2, 2)",
    "ValueError: latent mask must be [3, 1, 2, 2], got (3, 1, 4, 4)",
    "ValueError: mask values must lie in [0, 1]",
    "ValueError: attn_ctrl must carry one control per sample (3), got 2",
)


@pytest.fixture(scope="module")
def runs():
    return {name: tc.run_case(*c) for name, c in tc.cases().items()}


def test_translate_makes_the_recorded_engine_calls(runs):
    with open(tc.FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(runs)
    bad = [name for name in runs if runs[name][0] != want[name]]
    for name in bad[:3]:
        print("---- %s\nrecorded: %s\nnow: %s" % (name, json.dumps(want[name]), json.dumps(runs[name][1], indent=1)))
    assert not bad, "%d of %d cases differ from the fixture, the first: %s" % (len(bad), len(runs), bad[:10])


def _coupled_calls(full):
    """(method, samples of the call's chunk, members folded into the call) of every coupled engine call"""
    out = []
    for name, args, kw in full["calls"]:
        if name in tc.COUPLED:
            kw = dict(kw)
            nb = args[5][1][0] if name == "cycle_translate_masked" else kw["mapper"][1][0] if "mapper" in kw else tc.BSZ
            out.append((name, nb, args[2][1][0] // nb))
    return out


def test_the_grid_reaches_what_it_is_there_to_pin(runs):
    cases = tc.cases()
    done = [n for n in runs if isinstance(runs[n][0]["result"], list)]
    raised = [n for n in runs if isinstance(runs[n][0]["result"], str)]
    assert len(runs) == 243 and len(done) == 178 and len(raised) == 65 and len(done) + len(raised) == len(runs)
    grid = [n for n in runs if not n.startswith("x-")]
    assert len(grid) == 210 and len(set(grid) & set(done)) == 154
    # every precondition's text is raised by some case, and nothing else is
    texts = {runs[n][0]["result"] for n in raised}
    assert len(texts) == len(PRECONDITIONS)
    for p in PRECONDITIONS:
        assert any(t.startswith(p) for t in texts), p
    for n in raised:  # a precondition calls nothing and leaves last_translate_coupled alone (the control's batch is checked later)
        assert runs[n][0]["methods"] == [], n
        assert runs[n][0]["coupled"] == (True if runs[n][0]["result"].startswith(PRECONDITIONS[-1]) else "untouched"), n
    # each coupled engine method: several member chunks of one group, and - where the loop may cut the batch: a mask held to
    # the encoder, or control - several sample chunks; the plain path couples only while the whole batch fits
    sample_chunked, member_chunked, n_calls = set(), set(), set()
    for n in done:
        calls = _coupled_calls(runs[n][1])
        n_calls.add(len(calls))
        for name, nb, members in calls:
            if nb < tc.BSZ:
                sample_chunked.add(name)
            if members == 1 and cases[n][0].get("fold_ensemble", True):  # a group is the 2 trials of one (scale, skip)
                member_chunked.add(name)
    assert member_chunked == set(tc.COUPLED)
    assert sample_chunked == {"cycle_translate_masked", "cycle_translate_ctrl"}
    assert {0, 2, 4, 8, 12} <= n_calls
    # the two-call fallback: taken by every mode that has one, never by the others
    for mode, (attrs, _auto, _masked) in tc.MODES.items():
        fell_back = [n for n in grid if n.split("-")[2] == mode and n in done and runs[n][0]["coupled"] is False]
        if "cac_steps" in attrs or attrs.get("mask_source") == "encoder":
            assert not fell_back, fell_back
        else:
            assert fell_back, mode
            assert all(not _coupled_calls(runs[n][1]) for n in fell_back)
