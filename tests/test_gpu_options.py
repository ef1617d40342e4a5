"""fs_set_option and the fetch entries of the eight per-step logs against recorded replies.  The fixture
tests/golden/option_replies.json holds, for every option, a script of calls -- accepted extremes, the first refused value
on either side, malformed values, every keyword, an unknown key -- put to one handle (one not yet in use, and for the
options that look at the engine one in use), with the return code, the error text of each refusal and the members
fs_get_int reads back after each call; and for every log at capacity 2 with two records the replies of the sizes-only call,
of a fetch with room for 1, for 2 and for all, and of the calls after the drain.  tools/record_option_replies.py recorded
them from the library of the commit before the options got one parser and the logs one fetch; this test replays the same
calls on the library as it is and wants the same replies, text for text.  8 x 6 x 5 cells; only the force, body-force
and residual logs take steps (two)."""
import json
import os

import pytest

import option_replies as R

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_replies.json")) as _f:
    RECORDED = json.load(_f)
OPTIONS = RECORDED["options"]


@pytest.fixture(scope="module")
def L():
    from fluid_simulation_amd import _lib
    return _lib.lib()


def test_fixture_is_what_this_test_reads():
    assert RECORDED["readback"] == R.READBACK and sorted(RECORDED["logs"]) == sorted(R.LOGS)
    assert len(OPTIONS) > 63 and all(len(o["calls"]) == len(o["replies"]) >= 3 for o in OPTIONS)
    replies = [r for o in OPTIONS for r in R.unpack(o, RECORDED["errors"])[1]]
    assert sum(r["rc"] != 0 for r in replies) > 300 and all(r["err"] for r in replies if r["rc"])
    assert all(len(r["ints"]) == len(R.READBACK) for r in replies)


@pytest.mark.parametrize("opt", OPTIONS, ids=["%s%s" % (o["name"], "-in-use" if o["engine"] else "") for o in OPTIONS])
def test_option_replies(L, opt):
    script, replies = R.unpack(opt, RECORDED["errors"])
    got = R.run_script(L, script, opt["engine"])
    assert len(got) == len(replies)
    for call, g, want in zip(script, got, replies):
        print(call, g)
        assert g == want, (call, g, want)


@pytest.mark.parametrize("log", R.LOGS)
def test_log_fetch_replies(L, log):
    want = RECORDED["logs"][log]
    got = R.run_log(L, log)
    for g in got:
        print(g)
    assert len(want) >= 6 and want[0]["n"] >= 2 and want[1]["rc"] != 0 and want[1]["err"] and want[-1]["rc"] != 0
    assert [w["steps"] for w in want if w["steps"]] and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g, w)
