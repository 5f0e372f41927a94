"""CPU: the table of tests/video_matrix.py held to its claims, before any GPU time is spent on it.

  coverage   every pair of values of two different axes is in a row, or the product refuses the pair (`legal` on the pair
             with every other axis neutral, over every source); the same for every triple of (rate, retime, scene_cut,
             dedup).  The share of legal pairs and triples left uncovered is zero: a condition, not a measurement.
  refusals   every refusal `legal` reports is a ValueError that names the keyword of the axis to blame, raised before the
             output path exists (`legal` itself asserts the last part, for the streamed and the resident call)
  pinned     every pinned row is in the table and legal
  edges      for every dedup row and chunk size the chunk edges `_edges(n, C, look)` of tests/test_gpu_dedup_video.py cut
             a span of the row's pattern
  clips      the patterns' dead intervals, spans and cuts are what the comments beside them say
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402
import test_gpu_dedup_video as DV  # noqa: E402
import video_matrix as M  # noqa: E402

from ai_based_frame_interpolation_amd import retime  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    return M.rows()


def test_the_table_is_the_same_every_time(rows):
    M._rows = None
    try:
        again = M.rows()
    finally:
        M._rows = rows
    assert again == rows and len(set(rows)) == len(rows)
    assert all(M.canonical(r) == r for r in rows)
    n_product = len(M.product_rows())
    print(f"\n{len(rows)} rows: {n_product} of the product, {len(rows) - n_product} of the cover and the pinned rows")


def test_every_row_is_legal_and_every_axis_value_is_used(rows):
    assert all(M.is_legal(r) for r in rows)
    for axis, values in M.AXES.items():
        for v in values:
            assert any(getattr(r, axis) == v for r in rows), (axis, v)
    assert {r.source for r in rows} == set(M.SOURCES)
    assert any(r.precision == "fp32" for r in rows) and {r.clip for r in rows} == {"main", "two", "one"}


def test_every_legal_pair_and_triple_is_covered(rows):
    pairs, triples = set(), set()
    for r in rows:
        pairs |= M.pairs_of(r)
        triples |= M.triples_of(r)
    all_pairs = M.all_pairs()
    missing = [p for p in all_pairs if p not in pairs]
    refused = [p for p in missing if M.refused(p)]
    print(f"\npairs: {len(all_pairs)}, in a row: {len(all_pairs) - len(missing)}, refused by the product: {len(refused)}, "
          f"legal and uncovered: {len(missing) - len(refused)}")
    for p in refused:
        print("  refused pair:", dict(p))
    assert [p for p in missing if p not in refused] == []
    # a triple whose retime has no effect (no plan) is the triple with "blend": `canonical`
    all_triples, missing3 = M.all_triples(), []
    for t in all_triples:
        c = M.canonical(M.make(**dict(t)))
        t = tuple((a, getattr(c, a)) for a, _ in t)
        if t not in triples:
            missing3.append(t)
    refused3 = [t for t in missing3 if M.refused(t)]
    print(f"triples of {M.PRODUCT_AXES}: {len(all_triples)}, in a row: {len(all_triples) - len(missing3)}, refused by the "
          f"product: {len(refused3)}, legal and uncovered: {len(missing3) - len(refused3)}")
    assert [t for t in missing3 if t not in refused3] == []


def test_every_refusal_names_its_keyword(rows):
    M.rows()
    for p in M.all_pairs():      # (asks the product about every pair the table left out)
        if not any(p in M.pairs_of(r) for r in rows):
            M.refused(p)
    refusals = {k: v[1] for k, v in M._legal.items() if not v[0]}
    assert refusals, "the table met no refusal: the chroma axis alone has some"
    messages = {}
    for row, err in refusals.items():
        assert type(err) is ValueError, (M.row_id(row), type(err))
        blamed = M.blamed_axes(row)
        assert blamed, (M.row_id(row), "no single axis explains the refusal", str(err))
        for axis in blamed:
            assert any(k in str(err) for k in M.KEYWORD[axis]), (M.row_id(row), axis, str(err))
        messages.setdefault(str(err), []).append(row)
    print(f"\n{len(refusals)} refused combinations, {len(messages)} messages:")
    for msg, which in sorted(messages.items()):
        print(f"  {len(which):4d} x {msg}")
        print(f"         e.g. {M.row_id(which[0])}")


def test_pinned_rows_are_present_and_legal(rows):
    for name, row in M.PINNED.items():
        assert row in rows and M.is_legal(row), name
    p = M.PINNED
    assert p["motion-dedup8-cuts-y4m420"][:5] == ("y4m420-gray", "24to60-depth2", "motion", M.THR, (0, 8))
    assert p["chroma-motion-dedup-fps"].chroma == "motion" and p["chroma-motion-dedup-fps"].dedup is not None
    r = p["v210-area-dedup-cuts"]
    assert (r.source, r.resize, r.scene_cut) == ("v210", "area", M.THR) and r.dedup is not None
    r = p["rgb-y4m-dedup12-x4"]
    assert (r.source, r.rate, r.dedup) == ("y4m420-rgb", "x4", (1, 2))
    for name, fc in (("fp32-fps-dedup-cuts-gray", 1), ("fp32-fps-dedup-cuts-rgb", 3)):
        r = p[name]
        assert r.precision == "fp32" and M.SOURCES[r.source][1] == fc and "fps" in M.RATES[r.rate][1]
        assert r.dedup is not None and r.scene_cut is not None
    for name, clip in (("two-frames-dedup-cuts-fps", "two"), ("one-frame-dedup-cuts-fps", "one")):
        r = p[name]
        assert r.clip == clip and r.dedup is not None and r.scene_cut is not None and "fps" in M.RATES[r.rate][1]
        assert M.frames_of(r).shape[0] == (2 if clip == "two" else 1)


def test_the_clips_are_what_their_comments_say():
    for source in M.SOURCES:
        for dedup, pattern in (((0, 4), M.PATTERN), ((0, 8), M.PATTERN), ((1, 2), M.NOISE_PATTERN)):
            row = M.make(source=source, dedup=dedup, scene_cut=M.THR)
            frames = M.frames_of(row)
            assert frames.shape[0] == 23 == len(pattern) - 1
            dead, cuts = M.flags_of(row)
            letters = pattern.replace("|", "")
            assert dead == [letters[i] == letters[i + 1] for i in range(22)], (source, dedup)
            assert np.flatnonzero(cuts).tolist() == [pattern.index("|") - 1], (source, dedup)
            if dedup[0] == 1:     # near-repeats: dead at tolerance 1, and only there
                peaks = D.pair_peak(frames, M.bits_of(row))
                assert not any(D.dead_of(peaks, 0)) and all(0 < p <= 64 for p, d in zip(peaks, dead) if d)
    main = M.make(dedup=(0, 4))
    assert retime.dedup_spans(M.flags_of(main)[0], None, 4) == DV.SPANS + [(18, 2)]
    assert retime.dedup_spans(M.flags_of(main)[0], None, 8) == [(0, 2), (3, 3), (7, 4), (12, 5), (18, 2)]
    noise = M.make(dedup=(1, 2), scene_cut=M.THR)
    assert retime.dedup_spans(*M.flags_of(noise), 2) == [(2, 2), (4, 2)]
    assert retime.dedup_spans(M.flags_of(noise)[0], None, 2) == [(2, 2), (4, 2), (17, 2)]


def test_every_chunk_size_cuts_a_span(rows):
    checked = 0
    for row in rows:
        if row.dedup is None or row.clip != "main":
            continue
        dead, cuts = M.flags_of(row._replace(resize=None))     # (equal frames stay equal through a resize)
        spans = retime.dedup_spans(dead, cuts, row.dedup[1])
        assert spans, M.row_id(row)
        for C in M.chunk_sizes(row):
            edges = DV._edges(len(dead) + 1, C, M.look_of(row))
            assert any(a < s < a + ln for s in edges for a, ln in spans), (M.row_id(row), C, edges, spans)
            checked += 1
        assert row.dedup[1] + 1 in M.chunk_sizes(row)
    assert checked > 300
