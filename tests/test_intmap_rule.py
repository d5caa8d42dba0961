"""CPU suite of -i / --write_int_map: the host restatement (v2p_groups_intmap_json, csrc/host/group_muts.cpp) against the plain rule
(tests/intmap_rule.py), byte for byte, on the three golden VCFs, every non-panicking case of decode_cases.json and every case of
random_vcfs.json whose grouping does not abort; the rule's escaping against a table written from the grammar; the file-stem rule.

Counts of the fixtures as committed, checked with the rule alone: decode_cases.json has 13 cases, 9 of them marked `panics` (they
record the reference's aborts), and the rule raises ReferencePanic for none of the other 4: 4 are compared.  Half of that file cannot
be reached, so its bound is every non-`panics` case (4).  random_vcfs.json has 24 cases, none aborts: 24 are compared, and the bound
is half of the file."""
import json
import os

import pytest

import intmap_rule as J
from frontend_util import lists_to_arrays, oracle_lists

import frontend_oracle as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_files(text):
    """[(sample name, bytes)] by the host restatement, the lists taken from the oracle (no GPU)"""
    from vcf2prot_amd.frontend import Groups, HaplotypeLists, VcfIndex
    idx = VcfIndex(text.encode())
    hap_begin, ids = lists_to_arrays(oracle_lists(text)[4])
    g = Groups(idx, HaplotypeLists(hap_begin, ids))
    try:
        return [(name, g.intmap_json(s, name)) for s, name in enumerate(idx.sample_names())]
    finally:
        g.close()


def assert_host_equals_rule(text):
    want = J.int_maps_of_text(text)
    got = host_files(text)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert a == b, name
        obj = json.loads(a)                                             # every output parses
        assert list(obj) == ["proband_name", "mutations1", "mutations2"] and obj["proband_name"] == name
        for key in ("mutations1", "mutations2"):
            names = [g["name"].encode() for g in obj[key]]
            assert names == sorted(names) and len(set(names)) == len(names), (name, key)
    return len(got)


def test_rule_escaping_is_serde_jsons_for_every_byte_value():
    """json.dumps(ensure_ascii=False) on the one-character string of every code point below 256 equals E of the grammar (written out in
    intmap_rule.ESCAPES, not taken from a library); bytes from 0x80 are UTF-8 lead / continuation bytes and pass through E unchanged"""
    for c in range(256):
        want = J.escape_byte(c) if c < 0x80 else chr(c).encode()
        assert J.dumps(chr(c)) == b'"' + want + b'"', c
        if c >= 0x80:
            assert J.escape_byte(c) == bytes([c])
    assert J.E("Ké*".encode()) == "Ké*".encode()
    assert J.E(bytes(range(0x20))) == (b"\\u0000\\u0001\\u0002\\u0003\\u0004\\u0005\\u0006\\u0007\\b\\t\\n\\u000b\\f\\r\\u000e\\u000f"
                                       b"\\u0010\\u0011\\u0012\\u0013\\u0014\\u0015\\u0016\\u0017\\u0018\\u0019\\u001a\\u001b\\u001c\\u001d\\u001e\\u001f")


def test_library_escaping_equals_the_rule_for_every_byte_value(built):
    from vcf2prot_amd.frontend import json_escape
    for c in range(256):
        assert json_escape(bytes([c])) == J.escape_byte(c), c


@pytest.mark.parametrize("name", ["c1_example", "e2e_long", "e2e_dense"])
def test_host_restatement_equals_the_rule_on_the_golden_vcfs(built, name):
    text = open(os.path.join(GOLDEN, name + ".vcf")).read()
    assert assert_host_equals_rule(text) >= 1


@pytest.mark.parametrize("file,key,at_least", [("decode_cases.json", "panics", 4), ("random_vcfs.json", None, 12)])
def test_host_restatement_equals_the_rule_on_the_recorded_cases(built, file, key, at_least):
    """decode_cases.json: 13 cases, 9 `panics`, 0 ReferencePanic, 4 compared; random_vcfs.json: 24 cases, 24 compared"""
    cases = json.load(open(os.path.join(GOLDEN, file)))["cases"]
    compared = skipped = 0
    for c in cases:
        if key and c.get(key):
            skipped += 1
            continue
        try:
            J.int_maps_of_text(c["vcf"])
        except F.ReferencePanic:
            skipped += 1
            continue
        assert_host_equals_rule(c["vcf"])
        compared += 1
    print(file, "compared", compared, "skipped", skipped)
    assert compared + skipped == len(cases) and compared >= at_least


def test_a_group_without_members_and_an_extra_are_in_the_fixtures_or_written_here(built):
    """the two structural seams on VCF text: a transcript whose only consequence fails Mutation::new (a group with "alts":[]) and a
    consequence that joins another transcript's group through the substring match (transcript_name != name)"""
    head = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tP.1\tQ\n")
    rec = lambda pos, csq, a, b: f"1\t{pos}\t.\tA\tC\t.\tPASS\tBCSQ={csq}\tGT:BCSQ\t{a}\t{b}\n"
    text = (head + rec(10, "missense|G|ENSTX9|protein_coding|+|5A>5-C|10A>C", "0|1:2", "0|0:0") +
            rec(20, "missense|G|ENST12|protein_coding|+|7K>7*|20A>C", "1|1:3", "0|1:2") +
            rec(30, "missense|G|ENST1|protein_coding|+|9KL>9K*L|30A>C", "1|0:1", "0|0:0"))
    files = dict(J.int_maps_of_text(text))
    assert b'{"name":"ENSTX9","alts":[]}' in files["P.1"]                            # haplotype 2: only the consequence that does not parse
    assert b'{"name":"ENST1","alts":[{"transcript_name":"ENST12"' in files["P.1"]    # the extra
    assert b'"mutations1":[]' in files["Q"] and b'"NotSeq"' in files["Q"] and b'{"EndSequence":"K*L"}' in files["P.1"]
    assert_host_equals_rule(text)


def test_file_names_follow_set_extension():
    from vcf2prot_amd.frontend import int_map_file_name, int_map_name_refused
    want = {"A": "A.json", "A.1": "A.json", ".hidden": ".hidden.json", "A.b.c": "A.b.json", "NA1.2": "NA1.json", "A.": "A.json"}
    for name, file in want.items():
        assert J.file_name(name) == file and int_map_file_name(name) == file, name
        assert not J.refused(name) and not int_map_name_refused(name)
    assert int_map_file_name("A.1") == int_map_file_name("A.2")                      # the collision: one file, the later sample wins
    for name in ("", ".", "..", "a/b", "/x", "x/"):
        assert J.refused(name) and int_map_name_refused(name), name


def test_colliding_stems_share_a_file_and_the_later_sample_wins(built, tmp_path):
    from vcf2prot_amd.frontend import write_int_maps
    write_int_maps(str(tmp_path), ["A.1", "B", "A.2"], [b"one", b"two", b"three"])
    write_int_maps(str(tmp_path), ["B"], [b"again"])                               # the directory is reused
    d = tmp_path / "int_maps"
    assert sorted(os.listdir(d)) == ["A.json", "B.json"]
    assert (d / "A.json").read_bytes() == b"three" and (d / "B.json").read_bytes() == b"again"
