"""CPU: the library's request for hardware queues as a pure function (mnc_hw_queue_policy, csrc/ctx.hip): what GPU_MAX_HW_QUEUES
holds after the library was loaded, for every pairing of an exported value with a MNC_HW_QUEUES setting.  No HIP call, no GPU
process; no process is started at all, so none ever runs with a value above 32."""
import pytest

from mnc_amd import _lib

EXPORTED = [None, "4", "16", "24", "sixteen"]                    # absent / the runtime's own default / the request / more / garbage
SETTING = {None: 16, "0": 0, "2": 4, "8": 8, "64": 32, "many": 16}      # MNC_HW_QUEUES -> the request (0 = do not ask)


def _want(exported, setting):
    """The policy restated: a usable exported value is never lowered, a missing or lower one is set to the request."""
    have = int(exported) if exported is not None and exported.isdigit() and int(exported) > 0 else 0
    ask = SETTING[setting]
    if ask == 0:
        return have, "untouched"
    return (have, "kept") if have >= ask else (ask, "raised")


@pytest.mark.parametrize("setting", list(SETTING), ids=lambda s: "setting-%s" % s)
@pytest.mark.parametrize("exported", EXPORTED, ids=lambda e: "exported-%s" % e)
def test_policy_table(exported, setting):
    value, action = _lib.hw_queue_policy(exported, setting)
    assert (value, action) == _want(exported, setting)
    assert value <= 32
    if action == "raised":
        assert 4 <= value <= 32


def test_policy_spelled_out():
    """The rows the issue names, literally (independent of _want above)."""
    p = _lib.hw_queue_policy
    assert p(None, None) == (16, "raised")
    assert p("4", None) == (16, "raised")            # a lower exported value no longer wins
    assert p("16", None) == (16, "kept")
    assert p("24", None) == (24, "kept")             # never lowered
    assert p("sixteen", None) == (16, "raised")
    assert p("4", "0") == (4, "untouched")
    assert p(None, "0") == (0, "untouched")
    assert p(None, "2") == (4, "raised")             # clamp 2 -> 4
    assert p("4", "2") == (4, "kept")
    assert p(None, "64") == (32, "raised")           # clamp 64 -> 32
    assert p("24", "64") == (32, "raised")
    assert p("4", "8") == (8, "raised")
    assert p("16", "8") == (16, "kept")
    assert p("4", "many") == (16, "raised")          # text that is no integer counts as unset
    assert p("4", "") == (16, "raised")
    assert p(" 24 ", " 8 ") == (24, "kept")
    assert p("-3", None) == (16, "raised")
    assert p("4", "-1") == (4, "kept")               # an integer below the range is clamped like any other
    assert p("4", "99999999999999999999") == (32, "raised")        # ... and so is one too large for a long
    assert p(None, "-99999999999999999999") == (4, "raised")


def test_request_of_this_process_is_consistent():
    """mnc_hw_queue_request reports the hook of this very process: it agrees with the policy on what it says it found."""
    import os
    r = _lib.hw_queue_request()
    assert r["action"] in _lib.HWQ_ACTIONS
    assert (r["requested"] == 0) == (r["action"] == "untouched")
    assert r["requested"] == 0 or 4 <= r["requested"] <= 32
    before = None if r["exported_before"] is None else str(r["exported_before"])
    assert _lib.hw_queue_policy(before, os.environ.get("MNC_HW_QUEUES"))[1] == r["action"]
