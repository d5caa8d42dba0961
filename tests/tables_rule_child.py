"""Child process of test_gpu_tables_rule.py::test_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer filled
with 0xA5 when allocated, read once per process): the raw seam texts and a table of minimal size once more, every column equal to the
rule's.  A kernel that read memory it had not written (the slots, the counts, the prefix sums, the byte behind the aa bytes) would show
here.  Prints one line per case; the last line is "tables rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tables_rule as T  # noqa: E402
from test_gpu_tables_rule import run_raw  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for name, strings, caps in (("parse_shapes", T.parse_shapes(), None), ("aa_fields", T.aa_fields(), None), ("names", T.name_cases(), None),
                                    ("classes", T.class_cases(), (32, 16)), ("many_names", T.many_names(300), (512, 512)), ("empty", [""], None)):
            got, info = run_raw(ctx, strings, caps=caps)
            print(name, len(got["names"]), len(got["extra"]), len(got["aa"]), info["name_slots"], info["ident_slots"], flush=True)
    print("tables rule child ok", flush=True)


if __name__ == "__main__":
    main()
