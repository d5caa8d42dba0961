"""Child process of test_gpu_index_rule.py::test_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer filled with
0xA5 when allocated, the pads around the resident text with it; read once per process): the seam cases once more, every column and every
verdict equal to the rule's.  A kernel that counted bytes of the pad as text, or read a count or a prefix sum it had not written, would
show here.  Prints one line per case; the last line is "index rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import index_rule as R  # noqa: E402
from test_gpu_index_rule import check  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for name, text in R.seam_cases(R.TILE_BYTES) + R.item_cases()[:4] + R.order_cases():
            got = check(ctx, name, text)
            print(name, "refused" if got is None else len(got["row_begin"]), flush=True)
    print("index rule child ok", flush=True)


if __name__ == "__main__":
    main()
