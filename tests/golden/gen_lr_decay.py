"""Record what the reference's ``mae/lr_decay.py:param_groups_lrd`` returns for the models of
``tests/test_lr_decay_cpu.py`` (build container only: it imports the reference by path).

    python tests/golden/gen_lr_decay.py

Writes ``lr_decay.json`` next to this file: per case the keyword arguments and, per group, ``lr_scale``,
``weight_decay`` and the parameter NAMES in order -- names and numbers, nothing of the reference's source."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository
sys.dont_write_bytecode = True

from _ref_import import REF_ROOT  # noqa: E402
import test_lr_decay_cpu as T  # noqa: E402

spec = importlib.util.spec_from_file_location("_ref_lr_decay", os.path.join(REF_ROOT, "mae", "lr_decay.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

out = {}
for case in sorted(T.CASES):
    model, kw = T.build_case(case)
    groups = T.named_groups(model, ref.param_groups_lrd(model, **kw))
    out[case] = {"kwargs": kw, "groups": groups}
    print(f"{case}: {len(groups)} groups, {sum(len(g['params']) for g in groups)} parameters")
with open(os.path.join(HERE, "lr_decay.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
