"""Child process of test_gpu_resident_rows.py::test_resident_rows_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer
filled with 0xA5 when it is allocated AND whenever it is asked for again): the rows are staged once, so a buffer that is re-poisoned by a
later execute would show here.  Runs the module's first case -- both builders, first execute and three re-executes against the oracle."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    from sir_oracle import COracle
    from vcf2prot_amd.engine import Context

    from resident_rows_util import both_builders
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        both_builders(ctx, COracle())
    print("resident rows on poisoned memory: every haplotype is the oracle's", flush=True)


if __name__ == "__main__":
    main()
