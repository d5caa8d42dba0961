"""Sanitized fuzz of the BGZF inflater's decoder (vcf2prot_amd/csrc/inflate_format.hpp) on the host, before any corrupt input reaches the
GPU kernel that shares it.

    python tools/fuzz_inflate_host.py [--n 4000] [--seed 11]

Builds a small driver around inflate_format.hpp with g++ -fsanitize=address,undefined -fno-sanitize-recover, and feeds it the mutant corpus
of tests/inflate_corpus.py plus the valid members.  Every member is copied into a heap buffer of exactly its size, so a read past the
member's range is an ASan report; the status of every member must say "accepted" exactly where zlib's gzip decoder accepts it, with
zlib's bytes.  Prints one JSON line; exits non-zero on a sanitizer report or a disagreement.  CPU only."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_corpus as C  # noqa: E402

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "inflate_format.hpp"
struct W {
    uint32_t lane() const { return 0; } uint32_t size() const { return 1; } void sync() const {}
    uint64_t ballot(bool p) const { return p; } uint32_t popc(uint64_t m) const { return uint32_t(__builtin_popcountll(m)); }
    uint32_t rank(uint64_t) const { return 0; } uint32_t xor_all(uint32_t v) const { return v; }
};
int main(int argc, char** argv)
{
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = std::fopen(argv[2], "wb");
    infl::Scratch* s = new infl::Scratch;
    W w;
    infl::fill_crc_table(w, s->crc);
    uint32_t hdr[2];
    while (std::fread(hdr, 4, 2, f) == 2) {
        uint8_t* m = static_cast<uint8_t*>(std::malloc(hdr[0] ? hdr[0] : 1));      // exactly the member: ASan sees any read past it
        if (hdr[0] && std::fread(m, 1, hdr[0], f) != hdr[0]) return 3;
        const uint8_t* p = m;
        uint32_t done = 0;
        const uint32_t r = hdr[1] > infl::WINDOW ? uint32_t(infl::BAD_RANGE) : infl::inflate_member(w, *s, p, 0, hdr[0], hdr[1], &done);
        std::fwrite(&r, 4, 1, o);
        if (r == infl::OK) std::fwrite(s->window, 1, hdr[1], o);
        std::free(m);
    }
    delete s;
    std::fclose(f); std::fclose(o);
    return 0;
}
'''


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    corpus = C.mutants(a.n, a.seed) + [(name, m) for name, _, m in C.valid_members()]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "vcf2prot_amd", "csrc"), src, "-o", exe])
        inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(inp, "wb") as f:
            for _, m in corpus:
                f.write(struct.pack("<II", len(m), C.isize_of(m)) + m)
        p = subprocess.run([exe, inp, outp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        if p.returncode != 0:
            print(p.stderr[-4000:])
            print(json.dumps({"ok": False, "sanitizer_exit": p.returncode}))
            return 1
        out = open(outp, "rb").read()
    at, disagree, accepted, reasons = 0, [], 0, {}
    for name, m in corpus:
        r = struct.unpack_from("<I", out, at)[0]
        at += 4
        got = None
        if r == 0:
            got = out[at:at + C.isize_of(m)]
            at += C.isize_of(m)
            accepted += 1
        reasons[r] = reasons.get(r, 0) + 1
        want = C.zlib_member(m)
        if (got is None) != (want is None) or (got is not None and got != want):
            disagree.append(name)
    print(json.dumps({"ok": not disagree, "members": len(corpus), "accepted": accepted, "disagreements": disagree[:20],
                      "reasons": {str(k): v for k, v in sorted(reasons.items())}, "sanitizers": "address,undefined"}))
    return 0 if not disagree else 1


if __name__ == "__main__":
    sys.exit(main())
