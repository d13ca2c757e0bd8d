"""Status codes and messages of the C ABI's host-side checks against tests/golden/abi_errors.json (GPU, because ch_create needs one).

The golden table was written by tools/abi_error_digest.py from the library as it was BEFORE the entry points' common tail moved into
launch() / model_call() / workspace_short() (csrc/ch_api.cpp).  The same table of refused calls is replayed here; every status and
every message must be equal, so a message that changes by accident fails.  No case reaches a launch (see the tool)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest_tool():
    spec = importlib.util.spec_from_file_location('abi_error_digest', os.path.join(ROOT, 'tools', 'abi_error_digest.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_statuses_and_messages_equal_the_recorded_ones(hip_lib):
    from ctrlhair_amd import lib as L
    tool = _digest_tool()
    with open(os.path.join(ROOT, 'tests', 'golden', 'abi_errors.json')) as f:
        golden = json.load(f)
    got = tool.collect()
    assert [(r['entry'], r['case']) for r in got] == [(r['entry'], r['case']) for r in golden]       # the same table, in order
    diff = [(g, r) for g, r in zip(golden, got) if g != r]
    assert not diff, diff[:5]
    # the table is not a token one: a null-handle call of every entry point that takes a handle, and a refused call with one
    entries = tool.handle_entries(L.SYMBOLS)
    assert {r['entry'] for r in golden if r['case'] == 'null handle'} == set(entries)
    with_handle = {r['entry'] for r in golden if r['case'] != 'null handle'}
    assert set(entries) - with_handle == set(tool.NO_MESSAGE)
    # every workspace check: 12 sites, the PNG encoder's reached through both of its entry points
    assert sum('workspace smaller than' in r['message'] for r in golden) == 13
