"""tests/golden/reference_signatures.json: the call signatures of the reference classes the drop-in surfaces replace (parameter
name, kind, repr of the default), so that tests/test_reference_seams_cpu.py::test_signatures_equal_the_references can compare the
drop-ins with them where the reference is not installed.  Needs the reference checkout.

    python oracle/make_golden_signatures.py REFERENCE_ROOT
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SURFACES = {
    "SchedulerFlow": ("actionmesh.scheduler.scheduler", "SchedulerFlow",
                      ("__init__", "denoise", "get_noise", "get_schedule", "_flow_sample", "_compute_timesteps")),
    "ClassifierFreeGuidance": ("actionmesh.scheduler.guidance", "ClassifierFreeGuidance",
                               ("__init__", "get_unobserved_mask", "cfg_at_inference", "aggregate_cfg")),
    "ActionMeshDenoiser": ("actionmesh.model.temporal_denoiser", "ActionMeshDenoiser", ("__init__", "forward")),
    "AttentionProcessor": ("actionmesh.model.utils.attention_processor", "AttentionProcessor", ("__call__",)),
}


def signature_record(fn):
    return [[n, int(p.kind), None if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(fn).parameters.items()]


def main(ref_root):
    import importlib
    for p in (os.path.join(ROOT, "oracle", "diffusers_shim"), ref_root):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = {}
    for key, (mod, cls, methods) in SURFACES.items():
        klass = getattr(importlib.import_module(mod), cls)
        out[key] = {m: signature_record(getattr(klass, m)) for m in methods}
    path = os.path.join(ROOT, "tests", "golden", "reference_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
