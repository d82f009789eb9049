"""tests/golden/norm_bits.txt away from the card: it names exactly the cases of norm_bits_refs.cases (all of GN_CASES, their
table entries, every split-K case of GEMM_CASES with the three reduction kernels and both gnf forms among them), every case
lists the outputs its launch has, and the operand hashes reproduce here -- the fixture does not depend on where the operands
were built.  tests/test_norm_bits_gpu.py holds the library to the output hashes."""
import re

import kernel_refs as KR
import norm_bits_refs as N


def test_fixture_names_exactly_the_cases():
    _, rows = N.load()
    assert [(k, cid) for k, cid, _, _ in rows] == N.cases()
    gn = [cid for k, cid, _, _ in rows if k == "gn"]
    assert gn == [c["id"] for c in KR.GN_CASES] and len(gn) == 27
    assert [cid for k, cid, _, _ in rows if k == "table"] == [c["id"] for c in KR.GN_CASES if c["table"]]
    split = [KR.GEMM_CASE[cid] for k, cid, _, _ in rows if k == "splitk"]
    assert split == [c for c in KR.GEMM_CASES if c["splits"] > 1 and c["operands"] == "unit"] and len(split) == 63
    assert {c["reduce"] for c in split} == set(N.SPLITK_REDUCERS)
    assert {c["gnf"] for c in split} == {None, True, False}, "gnf with the raw result kept and skipped"


def test_every_case_lists_the_outputs_of_its_launch():
    _, rows = N.load()
    for kind, cid, hin, outs in rows:
        if kind != "splitk":
            want = {"y"} if kind == "gn" else {"table"}
        else:
            c = KR.GEMM_CASE[cid]
            want = {"out"} if c["gnf"] is None or c["gnf"] else set()
            want |= {k for k, on in (("gn_out", c["gn_out"]), ("ln_out", c["ln_out"]), ("gnf_y", c["gnf"] is not None)) if on}
        assert set(outs) == want, (cid, sorted(outs), sorted(want))
        assert all(re.fullmatch(r"[0-9a-f]{64}", h) for h in [hin, *outs.values()]), cid


def test_operand_hashes_reproduce():
    _, rows = N.load()
    bad = [cid for kind, cid, hin, _ in rows if N.input_hash(kind, cid) != hin]
    assert not bad, bad
