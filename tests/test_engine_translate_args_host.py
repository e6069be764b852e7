"""Engine.cycle_translate / cycle_translate_masked / cycle_translate_ctrl / ddim_decode_masked marshal their arguments into
the C entry points as tests/golden/engine_translate_args.json records (no GPU, a stand-in library: tests/_engine_translate_args.py).
The fixture was recorded while each of the three coupled forms had its own C entry point and its own copy of the marshalling;
the stand-in flattens today's one argument struct back to those positional lists."""
import json

import pytest

import _engine_translate_args as ea


@pytest.fixture(scope="module")
def runs():
    return {name: ea.run_case(*c) for name, c in ea.CASES.items()}


def test_the_c_entry_points_get_the_recorded_arguments(runs):
    with open(ea.FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(runs)
    for name in runs:
        assert runs[name][0] == want[name], name
    reached = {r[0]["symbol"] for r in runs.values() if "symbol" in r[0]}
    assert reached == set(ea.SYMBOLS)
    errors = {r[0]["error"] for r in runs.values() if "error" in r[0]}
    assert len(errors) == 11 and sum("error" in r[0] for r in runs.values()) == 15


def test_every_tensor_handed_to_the_library_outlives_the_call(runs):
    """the launches read them asynchronously: whatever the method converted or built is in `_keep`; the sampler's own input
    (x0 of the coupled forms, z of the decode) is the caller's argument and stays the caller's to hold"""
    for name, (rec, keep) in runs.items():
        if "symbol" in rec:
            passed, held = keep
            assert set(passed) - {"x0", "z"} <= set(held), (name, passed, held)
            assert len(passed) >= 2
