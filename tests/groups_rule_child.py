"""Child process of test_gpu_groups_rule.py::test_large_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer
filled with 0xA5 when allocated, read once per process): the large synthetic cases and the seam cases once more, every CSR array equal to
the rule's.  A kernel that read memory it had not written (the LDS bitmaps and prefixes, the counts, the refused flags, the bases) would
show here.  Prints one line per case and cap set; the last line is "groups rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import groups_rule as G  # noqa: E402
from test_gpu_groups_rule import LARGE, assert_kernel_equals_rule, decoded  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for name, make in list(LARGE.items()) + [("seams", G.case_seams)]:
            case = make()
            with decoded(ctx, case) as res:
                for caps in (None, (0, 1, 8192)):
                    info = assert_kernel_equals_rule(ctx, res, case, caps)
                    print(name, caps, info["lds_bytes"], info["n_groups"], info["n_members"], flush=True)
    print("groups rule child ok", flush=True)


if __name__ == "__main__":
    main()
