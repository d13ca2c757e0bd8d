"""Host half of the image ingest (ctrlhair_amd/ingest.py), CPU only: Pillow's BILINEAR coefficient tables applied in numpy equal
Pillow byte for byte, the other two oracles equal hostutil's resizes, and the batch packing round-trips."""
import numpy as np
import pytest

from ctrlhair_amd import hostutil as U
from ctrlhair_amd import ingest as G

from tests import ingest_oracle as IO

CASES = [(s, p) for s in IO.SHAPES for p in IO.SIZES] + IO.ONE_PASS


@pytest.mark.parametrize('shape,size', CASES, ids=[f'{h}x{w}-{p}' for (h, w), p in CASES])
def test_oracle_equals_pillow(shape, size):
    from PIL import Image
    for kind in ('random', 'ramp', 'white'):
        img = IO.content(kind, *shape)
        want = np.asarray(Image.fromarray(img).resize((size, size), Image.BILINEAR))
        got = IO.pil_resize_bilinear(img, size)
        assert got.shape == want.shape == (size, size, 3)
        assert np.array_equal(got, want), (kind, int((got != want).sum()))


def test_coefficient_tables():
    xmin, count, kk = G.pil_bilinear_coeffs(1024, 512)
    assert xmin.dtype == count.dtype == kk.dtype == np.int32 and kk.shape == (512, 5)           # support 2: ksize = 2 * 2 + 1
    assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= 1024).all() and (count <= kk.shape[1]).all()
    assert all((kk[i, count[i]:] == 0).all() for i in range(512))
    assert np.abs(kk.sum(1) - (1 << 22)).max() <= kk.shape[1]                                    # normalised, up to the roundings
    assert G.pil_bilinear_coeffs(1024, 512)[2] is kk                                             # cached
    assert G.pil_bilinear_coeffs(3, 512)[2].shape == (512, 3)                                    # enlarging: support 1
    assert G.pil_bilinear_coeffs(32768, 16)[2].shape == (16, 2 * 2048 + 1)
    for bad in ((0, 4), (4, 0), (32769, 4)):
        with pytest.raises(ValueError):
            G.pil_bilinear_coeffs(*bad)


@pytest.mark.parametrize('size', [32, 64])
def test_cv2_and_nearest_oracles_equal_hostutil(size):
    for shape in IO.SHAPES + [(size, size), (size, 40), (40, size)]:
        img = IO.content('random', *shape, seed=3)
        assert np.array_equal(IO.cv2_resize_linear(img, size), U.resize_bilinear(img, (size, size))), shape
        lab = (img[:, :, 0] % 19).astype(np.uint8)
        assert np.array_equal(IO.nearest(lab, size), U.resize_nearest(lab, (size, size))), shape


def test_sean_table_is_the_codes_jobs_arithmetic():
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    want = (np.transpose(ramp, [2, 0, 1]) / 127.5 - 1.0).astype(np.float32)[:, 0, :]            # preprocess_img's expression, then the cast
    assert np.array_equal(G.sean_lut(), want) and G.sean_lut().dtype == np.float32


def test_batch_packing_round_trips():
    shapes = [(100, 131), (64, 48), (100, 131), (32, 32), (32, 7), (9, 32)]
    addrs = [0x7F0000001000 + 4096 * i for i in range(len(shapes))]
    blob = G.pack_batch(addrs, shapes, 32, G.MODE_PIL_BILINEAR)
    assert blob.dtype == np.uint8 and blob.size % 16 == 0
    back = G.unpack_batch(blob, len(shapes))
    for a, (H, W), b in zip(addrs, shapes, back):
        assert (b['src'], b['H'], b['W']) == (a, H, W)
        assert (b['h'] is None) == (W == 32) and (b['v'] is None) == (H == 32)                   # a pass whose size stays is skipped
        for tab, n_in in ((b['h'], W), (b['v'], H)):
            if tab is not None:
                xmin, count, kk = G.pil_bilinear_coeffs(n_in, 32)
                assert tab[:2] == (n_in, 32)
                assert np.array_equal(tab[2], xmin) and np.array_equal(tab[3], count) and np.array_equal(tab[4], kk)
    # one table per distinct (in, out) pair and pass: the second 100 x 131 image adds nothing
    once = G.pack_batch(addrs[:2] + addrs[3:], shapes[:2] + shapes[3:], 32, G.MODE_PIL_BILINEAR)
    assert blob.size - once.size == G.DESC.itemsize
    # modes without tables: descriptors only
    for mode in (G.MODE_CV2_LINEAR, G.MODE_LABELS):
        b = G.pack_batch(addrs, shapes, 32, mode)
        assert b.size == len(shapes) * G.DESC.itemsize and all(d['h'] is None and d['v'] is None for d in G.unpack_batch(b, len(shapes)))
    for bad in (dict(shapes=[(0, 4)]), dict(shapes=[(4, 32769)]), dict(size=0), dict(size=4097), dict(mode=3), dict(shapes=[])):
        args = dict(addresses=addrs[:1], shapes=[(4, 4)], size=8, mode=0)
        args.update(bad)
        if not args['shapes']:
            args['addresses'] = []
        with pytest.raises(ValueError):
            G.pack_batch(**args)


def hostile_batches():
    """(case, blob, N, P, mode, accepted) for the library's host-side check of a batch: good ones, each documented refusal, and a good
    batch with single words overwritten (accepted = None: either answer, but no read outside the blob)."""
    good = G.pack_batch([4096, 8192, 12288], [(8, 6), (40, 1300), (4, 4)], 4, G.MODE_PIL_BILINEAR)
    labels = G.pack_batch([4096, 8192], [(8, 6), (512, 512)], 4, G.MODE_LABELS)
    yield 'good', good, 3, 4, 0, True
    yield 'good, fewer images than descriptors', good, 2, 4, 0, True
    yield 'labels', labels, 2, 4, G.MODE_LABELS, True
    yield 'cv2', labels, 2, 4, G.MODE_CV2_LINEAR, True
    yield 'widest row', G.pack_batch([4096], [(1, 32768)], 16, 0), 1, 16, 0, True
    yield 'N 0', good, 0, 4, 0, False
    yield 'N 65536', good, 65536, 4, 0, False
    yield 'P 0', good, 3, 0, 0, False
    yield 'P 4097', good, 3, 4097, 0, False
    yield 'mode 3', good, 3, 4, 3, False
    yield 'tables in mode 1', good, 3, 4, 1, False
    yield 'tables of another P', good, 3, 8, 0, False
    yield 'no tables in mode 0', labels, 2, 4, 0, False
    yield 'cut inside a table', good[:good.size - 16], 3, 4, 0, False
    yield 'cut inside the descriptors', good[:64], 3, 4, 0, False

    def edited(n, **fields):
        b = good.copy()
        d = b[:3 * G.DESC.itemsize].view(G.DESC)
        for k, v in fields.items():
            d[k][n] = v
        return b

    for case, b in (('H 0', edited(0, H=0)), ('W 32769', edited(1, W=32769)), ('null address', edited(2, src=0)),
                    ('table dropped', edited(0, htab=-1)), ('table of a skipped pass', edited(2, vtab=24)),
                    ('table offset past the end', edited(1, vtab=1 << 28)), ('table offset negative', edited(1, htab=-8)),
                    ('table offset not a multiple of 4', edited(0, htab=int(good[:32].view(G.DESC)['htab'][0]) + 1)),
                    ('table of another size', edited(0, W=7)), ('tables swapped', edited(0, htab=int(good[:32].view(G.DESC)['vtab'][0])))):
        yield case, b, 3, 4, 0, False
    rng = np.random.default_rng(11)
    for i in range(300):
        b = good.copy()
        w = b.view(np.int32)
        at = int(rng.integers(0, w.size))
        w[at] = int(rng.choice([-1, 0, 1, 2 ** 31 - 1, -2 ** 31, 65537, int(rng.integers(-2 ** 31, 2 ** 31))]))
        yield f'word {at} overwritten ({i})', b, 3, 4, 0, None


def test_workspace_query_checks_the_batch():
    """ch_ingest_workspace_bytes is the entries' own check, and host code: every hostile batch gets the documented answer here, without a
    GPU (tools/ingest_check_host.cpp runs the same cases under sanitizers)."""
    import ctypes
    import os
    from ctrlhair_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    query = lib.load().ch_ingest_workspace_bytes
    for case, blob, N, P, mode, accepted in hostile_batches():
        blob = np.ascontiguousarray(blob)
        need = int(query(blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, N, P, mode))
        if accepted is not None:
            assert (need > 0) == accepted, case
        if need:
            assert need % 256 == 0 and need >= blob.nbytes, case
    assert int(query(None, 0, 1, 4, 0)) == 0


def test_batch_check_under_sanitizers(tmp_path):
    """csrc/ingest_batch.h as a stand-alone CPU program under AddressSanitizer and UndefinedBehaviorSanitizer: the same cases; each
    batch is malloc'ed at its size, and for every batch that passes the program reads what the kernels would read from it."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clang = next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)), None) or shutil.which('clang++')
    assert clang, 'no ROCm clang++ to build tools/ingest_check_host.cpp with'
    exe = str(tmp_path / 'ingest_check_host')
    r = subprocess.run([clang, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                        os.path.join(root, 'tools', 'ingest_check_host.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    cases = list(hostile_batches())
    lines = []
    for i, (case, blob, N, P, mode, accepted) in enumerate(cases):
        path = str(tmp_path / f'{i:03d}.bin')
        np.ascontiguousarray(blob).tofile(path)
        lines.append(f'{path} {N} {P} {mode}')
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    r = subprocess.run([exe, str(tmp_path / 'list.txt')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, f'sanitizer report or failure (exit {r.returncode}):\n{r.stderr[-4000:]}'
    rows = r.stdout.splitlines()
    assert len(rows) == len(cases)
    for (case, blob, N, P, mode, accepted), row in zip(cases, rows):
        need, msg = row.split(' ', 1)
        assert (int(need) > 0) == (msg == 'ok'), (case, row)
        if accepted is not None:
            assert (msg == 'ok') == accepted, (case, row)
    said = {row.split(' ', 1)[1].split(': ')[-1] for row in rows}
    assert len(said) >= 12, said                                  # the overwritten words reach most of the refusals


def test_importing_the_host_half_needs_no_torch():
    import subprocess
    import sys
    code = ('import sys; sys.modules["torch"] = None\n'
            'from ctrlhair_amd import ingest as G\n'
            'G.pack_batch([4096], [(5, 7)], 4, 0); print("ok")')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=IO.__file__.rsplit('/tests/', 1)[0])
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]
