"""Record the call signatures of the reference's ``malstroem.algorithms.{fill,flow,label}`` functions that
``malstroem_amd.algorithms.hip.enable(target=...)`` rebinds (and of four flow functions it leaves alone) into
``tests/golden/reference_signatures.json``: module names, parameter names, kinds and defaults only, no code.

    python tests/golden/record_reference_signatures.py PATH/TO/REFERENCE/CHECKOUT
"""
import inspect
import json
import sys
from pathlib import Path

UNPATCHED = [("flow", "trace_accumulated_flow"), ("flow", "assign_watersheds_upstream"), ("flow", "upstream_cells"),
             ("flow", "trace_downstream")]


def main():
    sys.dont_write_bytecode = True                  # never write into the reference tree
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
    import malstroem.algorithms as ref_alg         # noqa: E402  (the reference)
    from malstroem.algorithms import fill, flow, label  # noqa: E402,F401
    from malstroem_amd.algorithms.hip import _PATCH
    out = {}
    for m, a in list(_PATCH) + UNPATCHED:
        fn = getattr(getattr(ref_alg, m), a)
        params = []
        for p in inspect.signature(fn).parameters.values():
            rec = {"name": p.name, "kind": p.kind.name}
            if p.default is not inspect.Parameter.empty:
                rec["default"] = p.default
            params.append(rec)
        out["%s.%s" % (m, a)] = {"module": fn.__module__, "patched": (m, a) in _PATCH, "params": params}
    path = Path(__file__).resolve().parent / "reference_signatures.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print("wrote", path, len(out), "functions")


if __name__ == "__main__":
    main()
