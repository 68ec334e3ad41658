"""The host side of the blocked gzip (BGZF) tests, no GPU: the model of tests/bgzf_files.py against Python's
own gzip reader on every well-formed file the builder makes, its member table against the builder's own
offsets, and the BSIZE arithmetic of ndfl.bgzf.compress on canned member lengths."""
import gzip
import struct

import pytest

import bgzf_files as B


@pytest.mark.parametrize("name,members", B.well_formed_files(), ids=[f[0] for f in B.well_formed_files()])
def test_model_equals_gzip(name, members):
    f = b"".join(members)
    m = B.model(f)
    assert m["status"] is None and m["bad_member"] == m["n_members"] == len(members)
    assert m["out"] == gzip.decompress(f) and m["out_len"] == len(m["out"]) == m["total"]
    assert m["table"] == B.offsets(members) and m["consumed_bytes"] == len(f)
    assert B.model(f, m["total"])["status"] is None
    if m["total"]:
        short = B.model(f, m["total"] - 1)
        assert short["status"] == B.E_CAPACITY and short["out_len"] == m["total"] and short["out"] == b""


def test_counts_reach_every_constant():
    c = B.constants()
    assert {"FIND_TILE", "FIND_THREADS", "FIND_BYTES", "LIST_TILE", "SUM_BLOCK", "LIST_MIN", "LIST_DIV"} <= set(c)
    assert c["FIND_TILE"] == c["FIND_THREADS"] * c["FIND_BYTES"]
    counts = B.member_counts()
    for t in (c["LIST_TILE"], c["SUM_BLOCK"], c["LIST_MIN"]):
        assert {t - 1, t, t + 1} <= set(counts)
    over = counts[-1]
    assert over > B.list_capacity(len(B.EMPTY) * over) and over - 1 <= B.list_capacity(len(B.EMPTY) * (over - 1))


def test_look_alikes_fill_more_list_tiles_than_a_sum_step():
    c = B.constants()
    f = b"".join([ms for name, ms in B.well_formed_files() if name.startswith("look-alikes")][0])
    at = [p for p in range(len(f) - 2) if f[p] == 0x1F and f[p + 1] == 0x8B and B.member_start(f, p)]
    members = [p for p, _, _ in B.chain(f)[0]]
    assert len(at) > c["SUM_BLOCK"] * c["LIST_TILE"] and len(at) > B.list_capacity(len(f))
    # members before and after the candidate that begins the sum kernel's second step
    assert at.index(members[5]) < c["SUM_BLOCK"] * c["LIST_TILE"] < at.index(members[-2])
    tiles = {name: -(-sum(map(len, ms)) // c["FIND_TILE"]) for name, ms in B.well_formed_files() if "scan tiles" in name}
    assert sorted(tiles.values()) == [c["SUM_BLOCK"] - 1, c["SUM_BLOCK"], c["SUM_BLOCK"] + 1, 2 * c["SUM_BLOCK"] + 1]
    assert all(name == f"{t} scan tiles" for name, t in tiles.items())


def test_member_start_rule():
    m = B.member(b"abc")
    assert B.member_start(m, 0) == len(m)
    assert B.member_start(m[:17], 0) is None                        # the extra field is cut
    assert B.member_start(m[:18], 0) == len(m)                      # the 12 + XLEN bytes are all it needs
    assert B.member_start(B.member(b"abc", flg=0), 0) is None
    assert B.member_start(B.member(b"abc", slen=3), 0) is None
    assert B.member_start(B.member(b"abc", ids=b"BX"), 0) is None
    assert B.member_start(B.member(b"abc", bsize=12 + 6 + 8 - 2), 0) is None          # BSIZE + 1 one below the minimum
    assert B.member_start(B.member(b"abc", bsize=12 + 6 + 8 - 1), 0) == 26
    assert B.member_start(b"\0" + m, 1) == len(m) and B.member_start(b"\0" + m, 0) is None


def test_chain_ignores_what_is_off_it():
    a, b = B.member(b"first"), B.member(b"second")
    fake = B.member(b"fake")
    stored = B.member(fake * 3, level=0)                            # look-alike headers in a stored payload
    f = a + stored + b + B.EOF
    assert fake in stored and len([p for p in range(len(f)) if B.member_start(f, p)]) == 7
    members, consumed = B.chain(f)
    assert [p for p, _, _ in members] == [0, len(a), len(a) + len(stored), len(f) - 28] and consumed == len(f)
    assert B.chain(b"junk" + f) == ([], 0)
    assert B.chain(f + b"junk")[1] == len(f)
    cut = f[:len(a) + 30]                                           # the second member's BSIZE runs past the end
    assert B.chain(cut) == ([(0, len(a), 5), (len(a), 30, struct.unpack("<I", cut[-4:])[0])], len(cut))
    assert B.model(cut)["status"] == "UNEXPECTED_END_OF_STREAM" and B.model(cut)["bad_member"] == 1


def test_first_error_wins():
    good = B.member(b"good" * 10)
    bad_crc = B.member(b"bad crc", crc=1)
    bad_size = B.member(b"bad size", isize=3)
    f = good + bad_size + bad_crc + good
    m = B.model(f)
    assert (m["status"], m["bad_member"], m["out_len"]) == (B.SIZE_MISMATCH, 1, 40 + 8)
    assert m["out"] == b"good" * 10 + b"bad"
    assert [t[1] for t in m["table"]] == [0, 40, 43, 50, 90]
    m = B.model(good + bad_crc + bad_size)
    assert (m["status"], m["bad_member"], m["out_len"]) == ("DECOMPRESSED_CHECKSUM_MISMATCH", 1, 47)


def test_patched_bsize():
    import ndfl.bgzf as Z
    head = bytes.fromhex("1f8b08040000000000ff060042430200") + b"\0\0"
    for n in (26, 28, 255, 256, 257, 65535, 65536):
        m = Z.member_with_bsize(head + bytes(n - len(head)))
        assert len(m) == n and m[16] | m[17] << 8 == n - 1 and m[:16] == head[:16] and m[18:] == bytes(n - 18)
        assert B.member_start(m, 0) == n
    with pytest.raises(ValueError):
        Z.member_with_bsize(head + bytes(65537 - len(head)))
    with pytest.raises(ValueError):
        Z.member_with_bsize(gzip.compress(b"no BC subfield"))
    assert Z.EOF == B.EOF and B.chain(Z.EOF) == ([(0, 28, 0)], 28)
