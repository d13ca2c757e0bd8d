"""CPU-only tests of the JPEG decoder's restart intervals: the marker parser (jpegdec.parse_jpeg_restart), the conditions the corpus of
tests/jpegdec_rst_cases.py must hold, its serial restatement against Pillow, and the entropy core (csrc/jpeg_entropy_core.h) run on the
CPU under AddressSanitizer and UndefinedBehaviorSanitizer by the stand-alone program tools/jpeg_entropy_host.cpp, over that corpus and
its malformed set."""
import io
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from ctrlhair_amd import jpegdec
from tests import jpegdec_cases as JC
from tests import jpegdec_oracle as JO
from tests import jpegdec_rst_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTART = 9


def _pillow(jpg: bytes, C: int) -> np.ndarray:
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.asarray(Image.open(io.BytesIO(jpg)).convert('RGB' if C == 3 else 'L'))


def test_corpus_conditions():
    RC.check_conditions()


def test_restatement_reproduces_pillow():
    for c, p, coef in RC.decoded():
        assert np.array_equal(JO.pixels(p, coef), _pillow(c.jpg, c.C)), c.name


def test_restatement_refuses_the_malformed_set():
    p = RC.tables_of(RC.malformed_base().jpg)
    assert RC.coefficients(p, 2).shape == (15 * 6, 64)
    for name, scan, ri in RC.malformed():
        with pytest.raises(JO.Bad):
            RC.coefficients(p._replace(scan=scan), ri)


def test_parse_jpeg_restart():
    assert jpegdec.STATUS_NAMES[RESTART] == 'RESTART' and len(jpegdec.STATUS_NAMES) == 10
    for c, p, coef in RC.decoded():
        H, W, C, sampling, tables, scan, ri = jpegdec.parse_jpeg_restart(c.jpg)
        assert (H, W, C, sampling, ri) == (c.H, c.W, c.C, c.sampling, c.ri), c.name
        assert scan == p.scan and len(RC.markers(scan)) == len(RC.RST.findall(c.jpg)), c.name     # the scan keeps its markers
        for k in range(C):
            assert np.array_equal(np.frombuffer(tables[64 * k:64 * k + 64], np.uint8), p.quant[k]), c.name
            for cls, (bits, vals) in ((0, p.dc[k]), (1, p.ac[k])):
                at = 192 + 272 * (2 * k + cls)
                assert tables[at:at + 16] == bits and tables[at + 16:at + 16 + len(vals)] == vals, c.name
        if ri:
            with pytest.raises(jpegdec.Unsupported, match=r'restart interval \(DRI\)'):                 # parse_jpeg keeps refusing them
                jpegdec.parse_jpeg(c.jpg)
        else:
            assert jpegdec.parse_jpeg(c.jpg) == (H, W, C, sampling, tables, scan)


def test_parse_jpeg_restart_equals_parse_jpeg_without_dri():
    for c in JC.corpus() + JC.sync_streams():
        assert jpegdec.parse_jpeg_restart(c.jpg) == jpegdec.parse_jpeg(c.jpg) + (0,), c.name
    for name, jpg in JC.malformed():
        try:
            want = jpegdec.parse_jpeg(jpg)
        except jpegdec.Unsupported as e:
            with pytest.raises(jpegdec.Unsupported, match='^' + __import__('re').escape(str(e)) + '$'):
                jpegdec.parse_jpeg_restart(jpg)
            continue
        assert jpegdec.parse_jpeg_restart(jpg) == want + (0,), name


def test_parse_jpeg_restart_refusals():
    base = RC.malformed_base()
    H, W, C, sampling, tables, scan, ri = jpegdec.parse_jpeg_restart(base.jpg)
    assert ri == 2
    at = base.jpg.index(scan)
    mid = len(scan) // 2
    while scan[mid - 1] == 0xFF or scan[mid] in (0, 0xFF):
        mid += 1
    with_c4 = base.jpg[:at + mid] + b'\xff\xc4' + base.jpg[at + mid:]
    with pytest.raises(jpegdec.Unsupported, match='marker FFC4 inside the scan'):
        jpegdec.parse_jpeg_restart(with_c4)
    dri = base.jpg.index(b'\xff\xdd')
    zero = base.jpg[:dri + 4] + b'\0\0' + base.jpg[dri + 6:]                     # DRI = 0: a restart marker in the scan is a marker as before
    for parse in (jpegdec.parse_jpeg, jpegdec.parse_jpeg_restart):
        with pytest.raises(jpegdec.Unsupported, match='marker FFD0 inside the scan'):
            parse(zero)
    with pytest.raises(jpegdec.Unsupported, match='bad DRI'):
        jpegdec.parse_jpeg_restart(base.jpg[:dri + 2] + b'\0\3' + base.jpg[dri + 4:dri + 6] + b'\0' + base.jpg[dri + 6:])
    with pytest.raises(jpegdec.Unsupported, match='no EOI'):
        jpegdec.parse_jpeg_restart(base.jpg[:-2])
    # the last DRI before the scan counts, as for libjpeg
    twice = base.jpg[:dri] + b'\xff\xdd\x00\x04\x00\x07' + base.jpg[dri:]
    assert jpegdec.parse_jpeg_restart(twice)[6] == 2


# ---- the entropy core on the CPU, under sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    clang = next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)), None) or shutil.which('clang++')
    assert clang, 'no ROCm clang++ to build tools/jpeg_entropy_host.cpp with'
    exe = str(tmp_path_factory.mktemp('entropy_rst_host') / 'jpeg_entropy_host')
    r = subprocess.run([clang, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                        os.path.join(ROOT, 'tools', 'jpeg_entropy_host.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_host(exe, work, items, rounds=0):
    """items: (H, W, C, sampling, tables, scan, Ri) -> [(status, launches needed, int16 [blocks, 64])]."""
    lines = []
    for k, (H, W, C, sampling, tables, scan, ri) in enumerate(items):
        for ext, data in (('scan', scan), ('tab', tables)):
            with open(os.path.join(work, f'{k}.{ext}'), 'wb') as f:
                f.write(data)
        lines.append(f'{work}/{k}.scan {work}/{k}.tab {H} {W} {C} {sampling} {rounds} {work}/{k}.out {ri}')
    lp = os.path.join(work, 'list.txt')
    with open(lp, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    r = subprocess.run([exe, lp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, f'sanitizer report or failure (exit {r.returncode}):\n{r.stderr[-4000:]}'
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(items)
    return [(int(st), int(needed), np.fromfile(os.path.join(work, f'{k}.out'), np.int16).reshape(-1, 64)) for k, (st, needed) in enumerate(rows)]


def test_entropy_core_under_sanitizers_corpus(host_program, tmp_path):
    cases = RC.decoded()
    res = run_host(host_program, str(tmp_path), [jpegdec.parse_jpeg_restart(c.jpg) for c, _, _ in cases])
    for (c, p, coef), (st, needed, got) in zip(cases, res):
        assert st == 0 and 1 <= needed <= 8, (c.name, st, needed)
        assert np.array_equal(got, coef), c.name
    # at every number of launches: the restatement's coefficients, or NOT_SYNCED
    multi = [(c, coef) for c, _, coef in cases if len(RC.scan_of(c.jpg)) > RC.CHUNK]
    assert len(multi) >= 2
    for rounds in (1, 2):
        res = run_host(host_program, str(tmp_path), [jpegdec.parse_jpeg_restart(c.jpg) for c, _ in multi], rounds=rounds)
        for (c, coef), (st, _, got) in zip(multi, res):
            assert st in (0, jpegdec.NOT_SYNCED) and (st or np.array_equal(got, coef)), (c.name, rounds, st)


def test_markers_end_the_walk_of_a_stream_without_eob(host_program, tmp_path):
    """Noise at quality 100 with optimised tables: every block holds 63 coefficients, no EOB lets the zigzag index re-synchronise, and
    the true state walks from chunk to chunk, one launch each.  Behind a restart marker every state is the true one."""
    px = JC.content('noise', 100, 131, 3, 0)
    needed = {}
    for name, kw in (('none', {}), ('b1', {'restart_marker_blocks': 1}), ('b7', {'restart_marker_blocks': 7}), ('rows', {'restart_marker_rows': 1})):
        p = jpegdec.parse_jpeg_restart(JC.save(px, quality=100, optimize=True, subsampling=0, **kw))
        assert len(p[5]) > 4 * RC.CHUNK
        st, needed[name], _ = run_host(host_program, str(tmp_path), [p])[0]
        assert st == 0, name
    assert needed['none'] >= 4 and max(needed['b1'], needed['b7'], needed['rows']) <= 2, needed


def test_entropy_core_under_sanitizers_malformed(host_program, tmp_path):
    base = jpegdec.parse_jpeg_restart(RC.malformed_base().jpg)
    bad = RC.malformed()
    assert len(bad) >= 20
    items = [base[:5] + (scan, ri) for _, scan, ri in bad]
    by_rounds = {rounds: [st for st, _, _ in run_host(host_program, str(tmp_path), [base] + items, rounds=rounds)] for rounds in (0, 1, 64)}
    for rounds, statuses in by_rounds.items():
        assert statuses[0] == 0, rounds                                        # the base itself
        got = dict(zip((n for n, _, _ in bad), statuses[1:]))
        assert all(got.values()), (rounds, got)                                # no accepted stream
    got = dict(zip((n for n, _, _ in bad), by_rounds[0][1:]))
    for name in ('markers-swapped', 'marker-number-changed', 'numbers-from-1', 'dri-1', 'dri-3', 'dri-4', 'marker-doubled',
                 'marker-doubled-next-number', 'marker-after-last-mcu'):
        assert got[name] == RESTART, (name, got[name])
    assert got['dri-0'] == got['dri-all']                                      # an interval that holds the whole scan: as without one
    for name in ('cut-after-marker', 'cut-after-first-marker', 'only-markers'):
        assert got[name] == 3, (name, got[name])                               # INPUT_END


def test_list_format_without_restart_column(host_program, tmp_path):
    """The list format of before (eight columns) means Ri = 0."""
    c = JC.corpus()[100]
    H, W, C, sampling, tables, scan = jpegdec.parse_jpeg(c.jpg)
    for ext, data in (('scan', scan), ('tab', tables)):
        with open(tmp_path / f'a.{ext}', 'wb') as f:
            f.write(data)
    with open(tmp_path / 'list.txt', 'w') as f:
        f.write(f'{tmp_path}/a.scan {tmp_path}/a.tab {H} {W} {C} {sampling} 0 {tmp_path}/a.out\n')
    r = subprocess.run([host_program, str(tmp_path / 'list.txt')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.split()[0] == '0', (r.stdout, r.stderr[-2000:])
