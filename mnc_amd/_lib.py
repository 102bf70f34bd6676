"""ctypes binding of libmnc_hip.so.  The prototypes are parsed from include/mnc_hip.h, so the Python side can never
drift from the C ABI.  There is NO fallback: if the library cannot be loaded, importing the device path raises."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "mnc_hip.h")
LIB_PATH = os.environ.get("MNC_LIB_PATH") or os.path.join(HERE, "libmnc_hip.so")    # MNC_LIB_PATH: an experiment build (tools/probes)

MNC_OK = 0


class MncError(RuntimeError):
    def __init__(self, code, func, msg):
        RuntimeError.__init__(self, "%s failed (status %d): %s" % (func, code, msg))
        self.code = code


_CTYPES = {
    "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
    "long": ctypes.c_long, "long long": ctypes.c_longlong,
    "void": None,
}


def _map_type(t):
    t = t.replace("const ", "").strip()
    if t.endswith("*"):
        return ctypes.c_void_p        # every pointer argument is passed as a raw address (host or device)
    return _CTYPES[t]


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes], [argnames])} for every MNC_API declaration."""
    with open(path) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"MNC_API\s+([\w\s\*]+?)\s*\b(\w+)\s*\(([^)]*)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        argtypes, argnames = [], []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                mm = re.match(r"(.+?)(\w+)$", a)
                argtypes.append(_map_type(mm.group(1)))
                argnames.append(mm.group(2))
        restype = ctypes.c_char_p if "char" in ret else _map_type(ret)
        decls[name] = (restype, argtypes, argnames)
    return decls


_lib = None
_decls = None


def load():
    """Load (building first if the .so is missing and hipcc is available).  Raises if that is impossible."""
    global _lib, _decls
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        from . import _build
        _build.build()
    lib = ctypes.CDLL(LIB_PATH)
    _decls = parse_header()
    for name, (restype, argtypes, _) in _decls.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch: fail loudly
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def call(name, *args):
    """Call an int-status entry point; raise MncError with mnc_last_error() on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != MNC_OK:
        raise MncError(rc, name, lib.mnc_last_error().decode("utf-8", "replace"))
    return rc


def ptr(a):
    """Address of a C-contiguous numpy array (kept alive by the caller), or pass-through for ints/None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
        return a.ctypes.data
    return a


def device_count():
    n = ctypes.c_int(0)
    call("mnc_device_count", ctypes.addressof(n))
    return n.value


def device_mem_info(device_id=0):
    """-> (free bytes, total bytes) of a device."""
    fr, tot = ctypes.c_size_t(0), ctypes.c_size_t(0)
    call("mnc_device_mem_info", int(device_id), ctypes.addressof(fr), ctypes.addressof(tot))
    return fr.value, tot.value


HWQ_ACTIONS = ("untouched", "kept", "raised")      # MNC_HWQ_UNTOUCHED / _KEPT / _RAISED (include/mnc_hip.h)


def _cstr(s):
    return None if s is None else ctypes.cast(ctypes.c_char_p(s.encode()), ctypes.c_void_p)


def hw_queue_policy(exported, setting):
    """The library's request for hardware queues as a pure function (mnc_hw_queue_policy): exported = GPU_MAX_HW_QUEUES, setting =
    MNC_HW_QUEUES, each a str or None (not in the environment) -> (value of GPU_MAX_HW_QUEUES afterwards, 0 = still absent;
    "untouched" | "kept" | "raised").  No HIP call."""
    value, action = ctypes.c_int(0), ctypes.c_int(0)
    e, s = _cstr(exported), _cstr(setting)
    call("mnc_hw_queue_policy", e, s, ctypes.addressof(value), ctypes.addressof(action))
    return value.value, HWQ_ACTIONS[action.value]


def hw_queue_request():
    """What the library's load-time hook did in this process -> {"requested": n (0: MNC_HW_QUEUES=0), "exported_before": the
    GPU_MAX_HW_QUEUES it found (None: absent or unusable), "action": "untouched" | "kept" | "raised"}.  No HIP call."""
    r, b, a = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    call("mnc_hw_queue_request", ctypes.addressof(r), ctypes.addressof(b), ctypes.addressof(a))
    return {"requested": r.value, "exported_before": None if b.value < 0 else b.value, "action": HWQ_ACTIONS[a.value]}


def stream_concurrency(n_streams, device_id=0):
    """How many of n_streams (1 .. 32) fresh streams run side by side on the device = the hardware queues they got, measured
    (mnc_stream_concurrency; a few milliseconds)."""
    n = ctypes.c_int(0)
    call("mnc_stream_concurrency", int(device_id), int(n_streams), ctypes.addressof(n))
    return n.value


_hw_queues = {}            # device -> stream_concurrency(32), NativeNet.hw_queues()
_family_probe = {}         # device -> (streams probed, concurrent) of check_hw_queues' last measurement
_hw_queues_warned = False


def hw_queues(device_id=0):
    """The hardware queues this process's streams get on the device: stream_concurrency(32), measured once per device and kept.
    Measure while the device is idle: a probe stream that shares a queue with a busy stream waits behind it, and the figure is
    then a lower bound."""
    if device_id not in _hw_queues:
        _hw_queues[device_id] = stream_concurrency(32, device_id)
    return _hw_queues[device_id]


def check_hw_queues(n_nets, device_id=0, who="nets"):
    """Warn, once per process, when n_nets streams of images in flight have fewer hardware queues than that: streams that share a
    queue serialise (profiles/hw_queues.txt: twelve images on four queues cost 5-6 %).  Changes nothing.  The measurement uses as many
    streams as the family has nets, not more, and is repeated as the family grows until one comes out short (that figure is the
    queue count and is kept).  Nets are added before images run, so the device is idle then; on a busy device the figure is a lower
    bound and the warning may be early.  -> the measured figure, or None for up to four nets: four queues are the runtime's own
    default and the floor of the library's request, only a host that exported fewer itself and set MNC_HW_QUEUES=0 has less, so
    nothing is measured for them."""
    global _hw_queues_warned
    if n_nets <= 4:
        return None
    probed, q = _family_probe.get(device_id, (0, 0))
    if q == probed and n_nets > probed:                       # (never short so far, and more nets than were ever tried)
        probed, q = min(n_nets, 32), stream_concurrency(min(n_nets, 32), device_id)
        _family_probe[device_id] = (probed, q)
    if q < probed and n_nets > q and not _hw_queues_warned:      # (a measurement that came out short: q is the queue count)
        _hw_queues_warned = True
        import warnings
        r = hw_queue_request()
        why = ("MNC_HW_QUEUES=0 left GPU_MAX_HW_QUEUES at %s" % r["exported_before"] if r["action"] == "untouched" else
               "the library asked for %d (GPU_MAX_HW_QUEUES %s), but the HIP runtime was initialised before libmnc_hip.so was loaded "
               "or grants fewer" % (max(r["requested"], r["exported_before"] or 0), r["action"]))
        warnings.warn("%d %s on GPU %d share %d hardware queue(s): streams on one queue run one after the other (%s); call "
                      "mnc_amd._lib.load() before anything else in the process uses HIP, or set MNC_HW_QUEUES / GPU_MAX_HW_QUEUES"
                      % (n_nets, who, device_id, q, why), RuntimeWarning, stacklevel=3)
    return q


def timing(entry_name, on):
    """One of the mnc_*_timing entries (boundary, polygons, accumulate, components): switch its event pair on or off -> the
    kernels' milliseconds of the last timed call before the switch (-1.0: none)."""
    last = ctypes.c_double(-1.0)
    call(entry_name, int(bool(on)), ctypes.addressof(last))
    return float(last.value)
