"""The CPU oracle's .pgen decoder on the directed files of tests/pgen_cases.py: record, difflist and header boundaries that neither the reference's example data
nor the random synthetic files reach.  Ground truth is the code matrix handed to the writer (3 -> -1); tests/test_gpu_pgen_edges.py holds the device decoder
to the same matrices, so every expectation there has two independent sources."""
import numpy as np
import pytest

import oracle_lib as ol
import pgen_cases as pc
import pgen_writer as pw


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    ol.build_oracle()


def test_the_case_list_covers_what_it_claims():
    names = set(pc.NAMES)
    assert {f"tails-{n}" for n in pc.TAILS} <= names and {f"idwidth-{n}" for n in pc.IDWIDTH} <= names
    assert {f"headers-{m}" for m in range(8)} <= names and {f"fixed-{n}" for n in (1, 4, 5, 13, 64)} <= names
    ids = pc.deltas_ids()
    widths = [len(pw.varint(int(d))) for d in np.diff(ids)]
    assert widths[:6] == [1, 2, 2, 3, 3, 4] and set(widths[64:127]) == {3} and set(widths[128:191]) == {3}
    g = pc.get("groups")
    lens = sorted({len(d[0] if isinstance(d, tuple) else d) for d in g.diff.values()})
    assert lens == [16384, 16385, 32769]
    b = pc.get("blocks-4bit")
    assert b.nv == 65536 + 71 and b.vrt[65535] in (2, 3) and b.vrt[65536] not in (2, 3) and b.vrt[65537] in (2, 3) and b.vrt[b.nv - 1] == 2
    ld = pc.get("ld")
    assert ld.vrt[-1] in (2, 3) and sorted(set(ld.vrt.tolist())) == [0, 1, 2, 3, 4, 6, 7]
    assert {a for a, _ in ld.windows} == set(range(ld.nv))                              # a window starts at every position of every run
    t = pc.get("tails-17")
    assert sorted(set(t.vrt.tolist())) == [0, 1, 2, 3, 4, 6, 7]
    ctrl = {int(pc.get(f"headers-{m}").img[11]) for m in range(8)}
    assert {c & 15 for c in ctrl} == set(range(8)) and {(c >> 4) & 3 for c in ctrl} == {0, 1, 2, 3} and {c >> 6 for c in ctrl} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", pc.NAMES)
def test_oracle_decodes_the_file_and_its_windows(name):
    c = pc.get(name)
    assert np.array_equal(ol.pgen_to_int8(c.img), c.want())
    for v0, v1 in c.windows:
        assert np.array_equal(ol.pgen_to_int8(c.img, v0, v1), c.want(v0, v1)), (v0, v1)
    v0, v1 = c.windows[0]
    rf, cf = pc.filters(c, v0, v1)
    assert np.array_equal(ol.pgen_to_int8(c.img, v0, v1, rf, cf), c.want(v0, v1, rf, cf))


@pytest.mark.parametrize("name", pc.NAMES)
def test_oracle_counts_genotypes(name):
    c = pc.get(name)
    assert np.array_equal(ol.pgen_geno_counts(c.img), c.counts())
    keep = pc.keep_mask(c)
    assert np.array_equal(ol.pgen_geno_counts(c.img, keep), c.counts(keep))


@pytest.mark.parametrize("name", pc.NAMES)
def test_dimensions(name):
    c = pc.get(name)
    assert ol.pgen_dims(c.img) == (c.ns, c.nv)


@pytest.mark.parametrize("name", [n for n in pc.MALFORMED if n not in pc.NOT_FOR_THE_ORACLE])
def test_oracle_refuses_malformed_files(name):
    img, _ = pc.malformed(name)
    with pytest.raises(ValueError):
        ol.pgen_to_int8(img)
