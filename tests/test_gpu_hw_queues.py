"""GPU: the library's request for hardware queues holds, and the measured count says so (csrc/ctx.hip, csrc/queue_probe.hip).

GPU_MAX_HW_QUEUES is read once, at a process's first HIP call, so every case is a fresh child process (this file run as a
program) with its own environment, one after another, each under a time limit; after a child that ends abnormally no further
child is started.  No child runs with more than 32 queues."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (GPU_MAX_HW_QUEUES exported to the child, MNC_HW_QUEUES or None = unset, streams probed, time limit in seconds)
CASES = {
    "a": ("4", None, 12, 120),
    "b": ("4", "0", 8, 120),
    "c": ("24", None, 12, 120),
    "d": ("4", None, 12, 300),
    "e": ("4", "0", 6, 300),
}
ABNORMAL = (124, 134, 137, 139)


def _child_probe(n_streams):
    from mnc_amd import _lib
    out = dict(_lib.hw_queue_request())
    out["concurrent"] = _lib.stream_concurrency(n_streams)
    return out


def _child_six_nets():
    """Six nets on one tiny weight set (reduced widths, the suite's smallest image size).  Twelve images are launched before the
    first fetch: a net takes its second image while its first is unfetched (the library first waits for that net's stream, the
    first image's results are overwritten), so the six fetches return images 6 .. 11.  Then all twelve go through the ring of six,
    image k + 6 launched as image k is fetched.  Everything must equal the same images run one at a time on one net."""
    import warnings
    from mnc_amd import _lib, models, synth
    from mnc_amd.native_net import NativeNet
    out = dict(_lib.hw_queue_request())
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=4)
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (75, 100, 3), dtype=np.uint8) for _ in range(12)]
    ref = NativeNet(w, use_graph=False)
    want = [ref.forward_image(im) for im in images]
    ref.close()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nets = [NativeNet(w)]
        nets += [NativeNet(nets[0]) for _ in range(5)]
    out["warnings"] = [str(c.message) for c in caught]
    out["hw_queues"] = nets[0].hw_queues()
    same = lambda a, b: bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True))
    for rounds in range(3):                              # eager, graph capture, graph replay -- each with twelve launches up front
        for k, im in enumerate(images):
            nets[k % 6].launch(im)
        got = [nets[k].fetch() for k in range(6)]
        out["launched_12_round%d" % rounds] = [same(want[6 + k], got[k]) for k in range(6)]
    got = []
    for k, im in enumerate(images):
        if k >= 6:
            got.append(nets[k % 6].fetch())
        nets[k % 6].launch(im)
    got += [nets[k % 6].fetch() for k in range(6, 12)]
    out["ring"] = [same(a, b) for a, b in zip(want, got)]
    out["rows"] = [int(c[0]) for c, _ in want]
    for n in reversed(nets):
        n.close()
    return out


def _child_six_nets_short_of_queues():
    """Six nets of one family in a process that opted out of the request and has the four exported queues: the fifth net's
    measurement comes out short, and exactly one warning names the cause."""
    import warnings
    from mnc_amd import _lib, models, synth
    from mnc_amd.native_net import NativeNet
    out = dict(_lib.hw_queue_request())
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=4)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nets = [NativeNet(w)]
        nets += [NativeNet(nets[0]) for _ in range(5)]
    out["warnings"] = [str(c.message) for c in caught if issubclass(c.category, RuntimeWarning)]
    for n in reversed(nets):
        n.close()
    return out


def _run_case(name):
    exported, setting, n_streams, limit = CASES[name]
    env = dict(os.environ, GPU_MAX_HW_QUEUES=exported)
    env.pop("MNC_HW_QUEUES", None)
    if setting is not None:
        env["MNC_HW_QUEUES"] = setting
    assert int(env["GPU_MAX_HW_QUEUES"]) <= 32 and int(env.get("MNC_HW_QUEUES", "0")) <= 32
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=REPO, env=env, timeout=limit,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    except subprocess.TimeoutExpired:
        return None, "case %s: the child ran into its time limit of %d s" % (name, limit)
    if r.returncode < 0 or r.returncode in ABNORMAL:
        return None, "case %s: the child ended abnormally (status %d)\n%s" % (name, r.returncode, r.stderr[-2000:])
    assert r.returncode == 0, "case %s: status %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), None


@pytest.fixture(scope="module")
def results():
    """Every case once, in order; the first abnormal end stops the sequence (the later cases then fail as 'not run')."""
    out, stopped = {}, None
    for name in sorted(CASES):
        if stopped:
            out[name] = (None, "not run: " + stopped)
            continue
        out[name] = _run_case(name)
        stopped = out[name][1]
    return out


def _get(results, name):
    res, err = results[name]
    assert err is None, err
    return res


@pytest.mark.gpu
def test_a_lower_exported_value_is_raised(results):
    r = _get(results, "a")
    assert (r["action"], r["requested"], r["exported_before"]) == ("raised", 16, 4)
    assert r["concurrent"] == 12                     # twelve streams, twelve queues


@pytest.mark.gpu
def test_b_opt_out_leaves_four_queues(results):
    r = _get(results, "b")
    assert (r["action"], r["requested"], r["exported_before"]) == ("untouched", 0, 4)
    assert r["concurrent"] == 4                      # eight streams share the four queues the host exported


@pytest.mark.gpu
def test_c_higher_exported_value_is_kept(results):
    r = _get(results, "c")
    assert (r["action"], r["requested"], r["exported_before"]) == ("kept", 16, 24)
    assert r["concurrent"] == 12


@pytest.mark.gpu
def test_d_six_nets_twelve_images_equal_one_at_a_time(results):
    r = _get(results, "d")
    assert r["action"] == "raised" and r["hw_queues"] == 16 and r["warnings"] == []
    assert sum(r["rows"]) > 0, "the images voted no instance at all: nothing was compared"
    for rounds in range(3):
        assert all(r["launched_12_round%d" % rounds]), (rounds, r["launched_12_round%d" % rounds])
    assert all(r["ring"]), r["ring"]


@pytest.mark.gpu
def test_e_six_nets_on_four_queues_warn_once(results):
    r = _get(results, "e")
    assert (r["action"], r["requested"], r["exported_before"]) == ("untouched", 0, 4)
    assert len(r["warnings"]) == 1, r["warnings"]
    msg = r["warnings"][0]
    assert "share 4 hardware queue(s)" in msg and "MNC_HW_QUEUES=0 left GPU_MAX_HW_QUEUES at 4" in msg
    assert msg.startswith("5 nets sharing one weight set on GPU 0")          # the fifth net is the first with no queue of its own


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    case = sys.argv[1]
    res = _child_six_nets() if case == "d" else _child_six_nets_short_of_queues() if case == "e" else _child_probe(CASES[case][2])
    print(json.dumps(res))
