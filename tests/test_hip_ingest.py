"""The image ingest on the HIP library (ch_ingest_images, ch_ingest_labels; ctrlhair_amd/ingest.py): every float of a ragged batch
against the host path it replaces, batch invariance, the ABI's refusals, and the masks and codes jobs with decode='device' against
decode='host'.  Equality throughout: the resizes are integer arithmetic, and the floats come out of a table the host path's own code
filled."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from ctrlhair_amd import dataset as D
from ctrlhair_amd import hostutil as U
from ctrlhair_amd import ingest as G
from ctrlhair_amd import lib as L
from tests import ingest_oracle as IO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def ing(handle):
    return G.ImageIngest(handle, DEV)


@pytest.fixture(scope='module')
def fp(handle):
    """FaceParsing without weights: normalise() and ingest_lut() need none."""
    from ctrlhair_amd.models import FaceParsing
    return FaceParsing(handle, DEV)


@pytest.fixture(scope='module')
def batch19():
    return [IO.content(kind, *shape) for kind, shape in IO.BATCH19]


def _host_parse_input(fp, images, P):
    from PIL import Image
    return torch.cat([fp.normalise(np.asarray(Image.fromarray(a).resize((P, P), Image.BILINEAR))) for a in images], dim=0)


def _dev(images):
    return [torch.from_numpy(a).to(DEV) for a in images]


@pytest.mark.parametrize('P', [16, 32, 62])
def test_parse_input_equals_the_host_path(ing, fp, batch19, P):
    """N = 19, every shape of the list in one ragged call; P = 62 is no multiple of 4: the scalar-store path."""
    want = _host_parse_input(fp, batch19, P)
    tensors = _dev(batch19)
    got = ing.parse_input(tensors, P, lut=fp.ingest_lut())
    assert got.dtype == torch.float32 and tuple(got.shape) == (19, 3, P, P)
    assert torch.equal(got, want), [n for n in range(19) if not torch.equal(got[n], want[n])]
    for n, t in enumerate(tensors):                               # image n of the batch is its N = 1 call
        assert torch.equal(ing.parse_input([t], P, lut=fp.ingest_lut())[0], got[n]), IO.BATCH19[n]


def test_parse_input_enlarging_to_512(ing, fp):
    img = IO.content('random', 100, 131)
    got = ing.parse_input(_dev([img]), 512, lut=fp.ingest_lut())
    assert torch.equal(got, _host_parse_input(fp, [img], 512))


def test_parse_input_skipped_passes_and_unaligned_sources(ing, fp):
    """W == P (the vertical pass reads the image itself, here from an address that is no multiple of 4), H == P, and both."""
    P = 32
    imgs = [IO.content('random', 37, P), IO.content('ramp', P, 37), IO.content('random', P, P), IO.content('random', 5, P, seed=1)]
    flat = torch.zeros(sum(a.size for a in imgs) + 8, dtype=torch.uint8, device=DEV)
    tensors, at = [], 1
    for a in imgs:                                                # packed back to back from byte 1: odd addresses
        flat[at:at + a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
        tensors.append(flat[at:at + a.size].view(a.shape))
        at += a.size
    assert any(t.data_ptr() % 4 for t in tensors)
    got = ing.parse_input(tensors, P, lut=fp.ingest_lut())
    assert torch.equal(got, _host_parse_input(fp, imgs, P))
    assert torch.equal(got[2], fp.normalise(imgs[2])[0])          # neither pass: just the table


@pytest.mark.parametrize('S', [32, 64])
def test_sean_input_and_labels_equal_preprocess(ing, batch19, S):
    """Mode 1 and the label resize against HairEditor.preprocess_img / preprocess_mask after the codes job's casts; the label maps have
    other sizes than their images (twice the image size: the 512 x 512 maps beside 256 x 256 crops)."""
    want = torch.from_numpy(np.concatenate([(np.transpose(U.resize_bilinear(a, (S, S)), [2, 0, 1]) / 127.5 - 1.0)[None] for a in batch19])
                            .astype(np.float32))
    got = ing.sean_input(_dev(batch19), S)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(ing.sean_input(_dev(batch19[4:5]), S)[0], got[4])
    rng = np.random.default_rng(5)
    maps = [rng.integers(0, 19, (2 * S, 2 * S), dtype=np.uint8)] + [rng.integers(0, 19, s, dtype=np.uint8) for s in IO.SHAPES[:5]] + \
           [rng.integers(0, 19, (S, S), dtype=np.uint8)]
    labs = ing.labels(_dev(maps), S)
    assert labs.dtype == torch.uint8 and tuple(labs.shape) == (len(maps), S, S)
    for n, m in enumerate(maps):
        assert np.array_equal(labs[n].cpu().numpy(), U.resize_nearest(m, (S, S))), m.shape
    assert torch.equal(ing.labels(_dev(maps[:1]), S)[0], labs[0])


def test_abi_refusals(handle, ing, fp):
    lib = handle.lib
    img = torch.zeros((8, 6, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 4, 4), -7.0, device=DEV)
    lab_out = torch.full((1, 4, 4), 77, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    lut = fp.ingest_lut()
    good = G.pack_batch([img.data_ptr()], [(8, 6)], 4, 0)
    err = lambda: lib.ch_last_error(handle._h).decode()

    def images(blob=good, nbytes=None, N=1, P=4, mode=0, lut_p=lut.data_ptr(), out_p=out.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=ws.numel()):
        b = None if blob is None else blob.ctypes.data_as(ctypes.c_void_p)
        rc = lib.ch_ingest_images(handle._h, b, (0 if blob is None else blob.nbytes) if nbytes is None else nbytes, N, P, mode, lut_p, out_p,
                                  ws_p, ws_bytes, None)
        return rc, err()

    def edited(**fields):
        b = good.copy()
        d = b[:G.DESC.itemsize].view(G.DESC)
        for k, v in fields.items():
            d[k][0] = v
        return b

    def table_word(at, value):                                   # one int32 of the horizontal table, `at` words behind its start
        b = good.copy()
        b.view(np.int32)[int(b[:32].view(G.DESC)['htab'][0]) + at] = value
        return b

    need = int(lib.ch_ingest_workspace_bytes(good.ctypes.data_as(ctypes.c_void_p), good.nbytes, 1, 4, 0))
    assert need >= good.nbytes + 8 * 4 * 3 and need % 256 == 0
    for change, word in ((dict(blob=None), 'null pointer'), (dict(lut_p=None), 'null pointer'), (dict(out_p=None), 'null pointer'),
                         (dict(ws_p=None), 'null pointer'), (dict(N=0), 'N outside'), (dict(N=65536), 'N outside'),
                         (dict(P=0), 'output side outside'), (dict(P=4097), 'output side outside'), (dict(mode=2), 'mode is not 0 or 1'),
                         (dict(mode=-1), 'mode is not 0 or 1'), (dict(out_p=out.data_ptr() + 4), '16-byte aligned'),
                         (dict(ws_p=ws.data_ptr() + 16), '256-byte aligned'), (dict(ws_bytes=need - 1), 'ch_ingest_workspace_bytes'),
                         (dict(nbytes=16), 'shorter than N descriptors'), (dict(N=2), 'image 1: '),
                         (dict(blob=edited(H=0)), 'image 0: side outside'), (dict(blob=edited(W=32769)), 'image 0: side outside'),
                         (dict(blob=edited(src=0)), 'image 0: null address'), (dict(blob=edited(htab=-1)), 'image 0: a table where'),
                         (dict(blob=edited(W=4)), 'image 0: a table where'), (dict(blob=edited(vtab=1 << 20)), 'vertical table offset'),
                         (dict(blob=edited(W=7)), 'horizontal table is not the one'), (dict(blob=table_word(2, 0)), 'ksize'),
                         (dict(blob=table_word(4, -1)), 'taps outside the image'), (dict(blob=table_word(4 + 2 * 3, 6)), 'taps outside the image'),
                         (dict(blob=table_word(5, 99)), 'taps outside the image'), (dict(P=16), 'table is not the one')):
        rc, msg = images(**change)
        assert rc == ERR_ARG and msg.startswith('ch_ingest_images: ') and word in msg, (change.keys(), rc, msg)
    assert lib.ch_ingest_images(None, good.ctypes.data_as(ctypes.c_void_p), good.nbytes, 1, 4, 0, lut.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                ws.numel(), None) == ERR_ARG       # a null handle

    lab = torch.zeros((8, 6), dtype=torch.uint8, device=DEV)
    lgood = G.pack_batch([lab.data_ptr()], [(8, 6)], 4, G.MODE_LABELS)

    def labels(blob=lgood, N=1, S=4, out_p=lab_out.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=ws.numel()):
        b = None if blob is None else blob.ctypes.data_as(ctypes.c_void_p)
        return lib.ch_ingest_labels(handle._h, b, 0 if blob is None else blob.nbytes, N, S, out_p, ws_p, ws_bytes, None), err()

    for change, word in ((dict(blob=None), 'null pointer'), (dict(out_p=None), 'null pointer'), (dict(ws_p=None), 'null pointer'),
                         (dict(N=0), 'N outside'), (dict(S=0), 'output side outside'), (dict(S=4097), 'output side outside'),
                         (dict(ws_p=ws.data_ptr() + 8), '256-byte aligned'), (dict(ws_bytes=255), 'ch_ingest_workspace_bytes'),
                         (dict(blob=good), 'a table where')):
        rc, msg = labels(**change)
        assert rc == ERR_ARG and msg.startswith('ch_ingest_labels: ') and word in msg, (change.keys(), rc, msg)
    # the size query: 0 for whatever the entries refuse
    q = lambda blob, N, P, mode: int(lib.ch_ingest_workspace_bytes(None if blob is None else blob.ctypes.data_as(ctypes.c_void_p),
                                                                   0 if blob is None else blob.nbytes, N, P, mode))
    assert q(lgood, 1, 4, G.MODE_LABELS) == 256 and q(good, 1, 4, 1) == 0 and q(lgood, 1, 4, 1) == 256
    for args in ((None, 1, 4, 0), (good, 0, 4, 0), (good, 1, 0, 0), (good, 1, 4097, 0), (good, 1, 4, 3), (good, 2, 4, 0), (edited(H=32769), 1, 4, 0)):
        assert q(*args) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((lab_out == 77).all()) and not bool(ws.any())          # nothing ran
    # and the handle is as usable as before
    assert torch.equal(ing.parse_input([img], 4, lut=lut), _host_parse_input(fp, [img.cpu().numpy()], 4))


# ---- the jobs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def job(hip_lib, tmp_path_factory):
    """The editor of tests/test_dataset.py (procedural weights) and a directory of five files, 64 to 256 pixels: 4:2:0 and 4:4:4 JPEGs,
    two PNGs and a BMP, which no decoder takes."""
    from PIL import Image
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import HairEditor, procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, 16)
    he = HairEditor(True, True, weights=w, device=0, img_size=256, max_batch=2)
    root = tmp_path_factory.mktemp('ingest_job')
    img_dir = root / 'images'
    img_dir.mkdir()
    base = ((P.synthetic_images(5, 256, seed=33).transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).astype(np.uint8)
    Image.fromarray(base[0]).save(img_dir / '00.jpg', quality=90, subsampling=2)
    Image.fromarray(base[1][:131, :100]).save(img_dir / '01.jpg', quality=85, subsampling=0)
    Image.fromarray(base[2][:64, :64]).save(img_dir / '02.png')
    Image.fromarray(base[3][:150, :200]).save(img_dir / '03.png')
    Image.fromarray(base[4][:96, :80]).save(img_dir / '04.bmp')
    return he, root, str(img_dir)


def _dir_bytes(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def test_masks_job_decode_device_writes_the_same_labels(job):
    he, root, img_dir = job
    host, dev, dev_png = (str(root / n) for n in ('label_host', 'label_dev', 'label_dev_png'))
    stats = {}
    assert D.extract_masks(he, img_dir, host, batch=2) == D.list_images(img_dir)
    assert D.extract_masks(he, img_dir, dev, batch=2, decode='device', stats=stats) == D.list_images(img_dir)
    assert stats == {'fallbacks': 1}                             # the .bmp
    a, b = _dir_bytes(host), _dir_bytes(dev)
    assert sorted(a) == [f'{i:02d}.png' for i in range(5)] and a == b          # png='host': the same file bytes
    D.extract_masks(he, img_dir, dev_png, batch=2, decode='device', png='device')
    for n in a:
        want = D.read_gray(os.path.join(host, n))
        assert want.shape == (512, 512) and np.array_equal(D.read_gray(os.path.join(dev_png, n)), want), n
    stats = {}
    D.extract_masks(he, img_dir, str(root / 'label_host2'), batch=2, stats=stats)
    assert stats == {'fallbacks': 0}


def test_codes_job_decode_device_agrees_with_host(job):
    he, root, img_dir = job
    label_dir = str(root / 'label_for_codes')
    D.extract_masks(he, img_dir, label_dir, batch=2)
    stats = {}
    host = D.encode_sean_codes(he, img_dir, label_dir, str(root / 'codes_host'), 'ds', batch=2)
    dev = D.encode_sean_codes(he, img_dir, label_dir, str(root / 'codes_dev'), 'ds', batch=2, decode='device', stats=stats)
    assert stats == {'fallbacks': 1}
    assert sorted(host) == sorted(dev) == [f'ds___{i:02d}' for i in range(5)]
    assert sorted(os.listdir(root / 'codes_host')) == sorted(os.listdir(root / 'codes_dev')) == [f'ds___{i:02d}.pkl' for i in range(5)]
    for k in host:
        with open(root / 'codes_dev' / (k + '.pkl'), 'rb') as f:
            c = pickle.load(f)
        assert type(c) is np.ndarray and c.shape == (19, 512) and c.dtype == np.float32 and np.array_equal(c, dev[k])
        d = float(np.abs(c - host[k]).max())
        print(f'{k}: max |device - host| = {d:.3e}')
        assert d <= 1e-5
