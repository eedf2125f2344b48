#!/usr/bin/env python3
"""what the executor planner makes of the repo's five cfgs, as the existing capi calls show it: kernel_count, arena_bytes, the step_model() list and
(FFGPU_KEEP_ALL) the layers read_layer accepts, per case.  `python tools/plan_pin.py` records tests/data/plan_pin.json on an MI355X;
tests/planner/test_gpu_cfg_styles.py imports CASES and record() and compares.  Create only: no forward runs, so the weights do not matter (the test cfgs load
without a .weights file: zero filters)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PIN = os.path.join(ROOT, "tests", "data", "plan_pin.json")
YOLO = "yolo-fastest-1.1.cfg"
CFGS = [YOLO, "dark3.cfg", "group3.cfg", "mini.cfg", "tiny3.cfg"]
FLAGS = ["0", "NO_FUSE", "KEEP_ALL", "CONCURRENT", "SPLIT2"]

# (cfg, batch, flags name, environment): batch 1 patches the batch input into add steps, 2 inserts the CNHW conversion and allows a split, 3 refuses it
CASES = [(c, b, f, {}) for c in CFGS for b in (1, 2, 3) for f in FLAGS if f != "SPLIT2" or b == 2]
CASES += [(YOLO, b, "0", {k: "1"}) for k in ("FFGPU_BRANCH", "FFGPU_DWPW") for b in (1, 2, 3)]


def case_id(case):
    cfg, batch, flags, env = case
    return "%s b%d %s%s" % (cfg, batch, flags, "".join(" %s=%s" % kv for kv in sorted(env.items())))


def cfg_path(name):
    return os.path.join(ROOT, "data", name) if name == YOLO else os.path.join(ROOT, "tests", "data", name)


def record(capi, net, case):
    """the pinned values of one case (the caller has put the case's environment in place)"""
    _, batch, fname, _ = case
    flags = (0 if fname == "0" else getattr(capi.FFGPU, fname)) | capi.FFGPU.NO_GRAPH
    with net.executor(batch, flags) as ex:
        out = {"kernel_count": ex.kernel_count, "arena_bytes": ex.arena_bytes}
        if fname != "SPLIT2":
            out["steps"] = [[lay, by] for lay, by in ex.step_model()]
        if fname == "KEEP_ALL":
            ok = []
            for i in range(net.layer_num):
                try:
                    ex.read_layer(i, 0)
                    ok.append(i)
                except RuntimeError:
                    pass
            out["readable"] = ok
    return out


def record_all(capi, cases=CASES):
    out = {}
    for name in CFGS:
        with capi.Net(cfg_path(name), os.path.join(ROOT, "data", "yolo-fastest-1.1.weights") if name == YOLO else None) as net:
            for case in cases:
                if case[0] != name:
                    continue
                saved = {k: os.environ.get(k) for k in case[3]}
                os.environ.update(case[3])
                try:
                    out[case_id(case)] = record(capi, net, case)
                finally:
                    for k, v in saved.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
    return out


if __name__ == "__main__":
    from ffcnn_amd import capi
    pins = record_all(capi)
    with open(sys.argv[1] if len(sys.argv) > 1 else PIN, "w") as fp:              # one case per line
        fp.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(pins[k], sort_keys=True, separators=(",", ":"))) for k in sorted(pins)) + "\n}\n")
    print("%d cases -> %s" % (len(pins), fp.name))
