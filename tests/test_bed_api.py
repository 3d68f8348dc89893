"""scilmm_amd.bed.BedFile on the CPU: the fixed bytes of the format definition, a round trip through a packer written here,
the sample look-up and the errors of the constructor.  No GPU, no built library."""
import os

import numpy as np
import pytest

from scilmm_amd.bed import BedFile

CODE = {2: 0b00, -1: 0b01, 1: 0b10, 0: 0b11}        # A1 allele count -> the two bits of the file


def pack(G, pad_ones=True):
    """m x N int8 A1 counts (-1 = missing) as .bed rows: sample s in bits 2 (s & 3) .. of byte s >> 2, low bits first; the
    padding bits of the last byte set to ones (a reader that decoded them would see samples with no copy of A1)."""
    m, N = G.shape
    nb = (N + 3) // 4
    codes = np.full((m, 4 * nb), 0b11 if pad_ones else 0, dtype=np.uint8)
    for g, c in CODE.items():
        codes[:, :N][G == g] = c
    q = codes.reshape(m, nb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def write_fileset(prefix, packed, N, iids=None, magic=b"\x6c\x1b\x01", extra=b""):
    prefix = str(prefix)
    iids = ["i%d" % s for s in range(N)] if iids is None else iids
    with open(prefix + ".fam", "w") as f:
        for s in range(N):
            f.write("fam%d %s 0 0 %d -9\n" % (s // 3, iids[s], 1 + s % 2))
    with open(prefix + ".bim", "w") as f:
        for j in range(packed.shape[0]):
            f.write("%d\trs%d\t%g\t%d\tA\tG\n" % (1 + j % 22, j, 0.5 * j, 1000 + j))
    with open(prefix + ".bed", "wb") as f:
        f.write(magic + packed.tobytes() + extra)
    return prefix


def random_genotypes(m, N, seed):
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(m, N)).astype(np.int8)
    G[rng.random((m, N)) < 0.1] = -1
    return G


FIXED = np.array([[2, 0, -1, 0, 0, 0], [0, -1, 1, 0, 0, 0], [0, 1, 1, -1, -1, 2]], dtype=np.int8)


def test_fixed_bytes_of_the_format_definition(tmp_path):
    prefix = str(tmp_path / "fixed")
    write_fileset(prefix, np.zeros((3, 2), np.uint8), 6)
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes.fromhex("6c1b01" "dc0f" "e70f" "6b01"))
    for path in (prefix, prefix + ".bed", prefix + ".fam"):
        bed = BedFile(path)
        assert (bed.n_samples, bed.n_markers) == (6, 3)
        G = bed.read()
        assert G.dtype == np.int8 and np.array_equal(G, FIXED)
    assert np.array_equal(bed.read(count="A2"), np.where(FIXED >= 0, 2 - FIXED, -1))
    assert bed.packed.shape == (3, 2) and bed.packed.dtype == np.uint8 and not bed.packed.flags.writeable
    assert isinstance(bed.packed, np.memmap) and bed.packed.tobytes() == bytes.fromhex("dc0fe70f6b01")
    assert list(bed.iid) == ["i%d" % s for s in range(6)] and list(bed.fid) == ["fam0"] * 3 + ["fam1"] * 3
    assert sorted(bed.bim) == ["a1", "a2", "chrom", "cm", "pos", "snp"]
    assert list(bed.bim["snp"]) == ["rs0", "rs1", "rs2"] and list(bed.bim["chrom"]) == ["1", "2", "3"]
    assert np.array_equal(bed.bim["pos"], [1000, 1001, 1002]) and np.array_equal(bed.bim["cm"], [0.0, 0.5, 1.0])
    assert list(bed.bim["a1"]) == ["A"] * 3 and list(bed.bim["a2"]) == ["G"] * 3
    with pytest.raises(ValueError):
        bed.read(count="B")


@pytest.mark.parametrize("N", [1, 3, 4, 5, 2003])
def test_round_trip(tmp_path, N):
    m = 23
    G = random_genotypes(m, N, N)
    bed = BedFile(write_fileset(tmp_path / "rt", pack(G), N))
    assert np.array_equal(bed.read(), G)
    assert np.array_equal(bed.read(count="A2"), np.where(G >= 0, 2 - G, -1))
    # a map: a permutation of the file's samples with some individuals absent, one sample used twice
    rng = np.random.default_rng(N + 1)
    idx = np.concatenate([rng.permutation(N), [-1, -1, 0]]).astype(np.int64)
    idx = idx[rng.permutation(idx.size)]
    want = np.where(idx >= 0, G[:, np.maximum(idx, 0)], -1)
    assert np.array_equal(bed.read(sample_index=idx), want)
    assert np.array_equal(bed.read(markers=slice(3, 20, 2), sample_index=idx), want[3:20:2])
    pick = np.array([22, 0, 7, 7, 5])
    assert np.array_equal(bed.read(markers=pick, sample_index=idx), want[pick])
    assert np.array_equal(bed.read(markers=pick), G[pick])
    assert bed.read(markers=slice(0, 0)).shape == (0, N)
    for bad in ([N], [-2], np.zeros((2, 2), int), [0.5]):
        with pytest.raises(ValueError):
            bed.read(sample_index=bad)
    with pytest.raises(ValueError):
        bed.read(markers=[m])


def test_sample_index(tmp_path):
    iids = ["carol", "alice", "dave", "bob", "erin"]
    bed = BedFile(write_fileset(tmp_path / "s", pack(random_genotypes(2, 5, 0)), 5, iids=iids))
    idx = bed.sample_index(["bob", "zed", "carol", "erin", "alice", "bob"])
    assert idx.dtype == np.int32 and np.array_equal(idx, [3, -1, 0, 4, 1, 3])
    assert np.array_equal(bed.sample_index(np.array(iids, dtype=object)), np.arange(5))
    assert bed.sample_index([]).shape == (0,)


def test_errors_name_the_file_and_the_reason(tmp_path):
    G = random_genotypes(4, 9, 1)
    P = pack(G)
    cases = [("magic", dict(magic=b"\x6c\x1c\x01"), "magic"),
             ("smajor", dict(magic=b"\x6c\x1b\x00"), "sample-major"),
             ("short", dict(packed=P.reshape(-1)[:-1].reshape(1, -1)), "truncated"),
             ("long", dict(extra=b"\x00"), "oversized"),
             ("dup", dict(iids=["a", "b", "c", "d", "b", "e", "f", "g", "h"]), "twice")]
    for name, kw, word in cases:
        prefix = str(tmp_path / name)
        packed = kw.pop("packed", P)
        write_fileset(prefix, P, 9, **{k: v for k, v in kw.items() if k == "iids"})      # .fam and .bim of the 4 x 9 file
        with open(prefix + ".bed", "wb") as f:
            f.write(kw.get("magic", b"\x6c\x1b\x01") + packed.tobytes() + kw.get("extra", b""))
        with pytest.raises(ValueError, match=word) as e:
            BedFile(prefix)
        assert os.path.basename(prefix) in str(e.value), name
    with open(str(tmp_path / "empty.bed"), "wb"):
        pass
    write_fileset(tmp_path / "ok", P, 9)
    os.replace(str(tmp_path / "empty.bed"), str(tmp_path / "ok.bed"))
    with pytest.raises(ValueError, match="ok.bed"):
        BedFile(str(tmp_path / "ok"))
