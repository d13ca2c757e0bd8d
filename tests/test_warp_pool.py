"""The adaptor warp pool job (ctrlhair_amd.dataset warp-pool): host logic with a fake warper, and three real pairs on the GPU."""
import os

import numpy as np
import pytest

from ctrlhair_amd import dataset as DS


class FakeWarper:
    """warp_batch returns the face labels with the donor's hair pasted as 13: enough to tell hair / face order and batching."""

    def __init__(self):
        self.calls = []

    def warp_batch(self, hair, face, hl, fl, mesher='host'):
        assert mesher == 'device'
        self.calls.append(len(hair))
        out = np.asarray(face).copy()
        out[np.asarray(hair) == 13] = 13
        return out


def _tree(tmp_path):
    root = tmp_path / 'root'
    labs = {}
    for k, (ds, name) in enumerate([('ffhq', '00011.png'), ('ffhq', '00012.png'), ('celeba', 'img_00007.png')]):
        os.makedirs(root / ds / 'label', exist_ok=True)
        lab = np.full((8, 8), k + 1, np.uint8)
        lab[k:k + 3, 2:5] = 13
        DS.write_label_png(str(root / ds / 'label' / name), lab)
        labs[(ds, name)] = lab
    lm = {'00011': np.full((81, 2), 0.25), 'ffhq___00012': np.full((81, 2), 0.5)}      # celeba/img_00007 has none
    return str(root), labs, lm


def test_pool_names_content_and_the_skipped_report(tmp_path, capsys):
    root, labs, lm = _tree(tmp_path)
    a, b, c = ('ffhq', '00011.png'), ('ffhq', '00012.png'), ('celeba', 'img_00007.png')
    w = FakeWarper()
    pool = str(tmp_path / 'pool')
    done, skipped = DS.warp_pool(w, root, pool, lm, [(a, b), (b, a), (c, a), (a, a)], batch=2)
    assert done == ['ffhq___00011___ffhq___00012___00.png', 'ffhq___00012___ffhq___00011___00.png', 'ffhq___00011___ffhq___00011___00.png']
    assert skipped == ['celeba/img_00007.png'] and 'no landmarks for celeba/img_00007.png' in capsys.readouterr().out
    assert w.calls == [2, 1] and sorted(os.listdir(pool)) == sorted(done)
    expect = labs[b].copy()
    expect[labs[a] == 13] = 13
    assert np.array_equal(DS.read_gray(os.path.join(pool, done[0])), expect)
    pool2 = str(tmp_path / 'pool_hair')
    done2, _ = DS.warp_pool(FakeWarper(), root, pool2, lm, [(a, b)], only_hair=True)
    assert np.array_equal(DS.read_gray(os.path.join(pool2, done2[0])), (expect == 13) * 255)
    assert DS.pool_name(c, a, 0) == 'celeba___00007___ffhq___00011___00.png'


def test_seeded_pairs_are_reproducible_and_sharded_without_overlap(tmp_path):
    root, _, lm = _tree(tmp_path)
    cands = DS.pool_candidates(root)
    assert cands == [('celeba', 'img_00007.png'), ('ffhq', '00011.png'), ('ffhq', '00012.png')]
    assert DS.pool_candidates(root, ['ffhq']) == cands[1:]
    p1, p2, p3 = DS.random_pairs(cands, 11, 5), DS.random_pairs(cands, 11, 5), DS.random_pairs(cands, 11, 6)
    assert p1 == p2 and p1 != p3 and len(p1) == 11 and all(h in cands and f in cands for h, f in p1)
    shards = [DS.shard(p1, r, 3) for r in range(3)]
    assert sorted(sum(shards, [])) == sorted(p1) and sum(len(s) for s in shards) == 11
    # the ranks write disjoint file sets: the rank is part of the name, and each rank takes every third pair
    have = cands[1:]
    pairs = DS.random_pairs(have, 7, 1)
    names = [set(DS.warp_pool(FakeWarper(), root, str(tmp_path / 'p'), lm, pairs, batch=4, rank=r, world=2)[0]) for r in range(2)]
    assert not (names[0] & names[1]) and len(names[0] | names[1]) == len({(p, k % 2) for k, p in enumerate(pairs)})


def test_pairs_file_parsing(tmp_path):
    f = tmp_path / 'pairs.txt'
    f.write_text('# hair face\nffhq 00011.png ffhq 00012.png\n\nceleba img_00007.png ffhq 00011.png\n')
    assert DS.read_pairs_file(str(f)) == [(('ffhq', '00011.png'), ('ffhq', '00012.png')), (('celeba', 'img_00007.png'), ('ffhq', '00011.png'))]
    f.write_text('ffhq 00011.png ffhq\n')
    with pytest.raises(ValueError, match='pairs.txt:1'):
        DS.read_pairs_file(str(f))


@pytest.mark.gpu
def test_three_real_pairs_equal_warp_batch(tmp_path):
    from ctrlhair_amd.warping import MaskWarper
    from tests.warp_cases import cases
    cs = cases()[:3]
    root = tmp_path / 'root'
    os.makedirs(root / 'fix' / 'label')
    lm = {}
    for k, c in enumerate(cs):
        DS.write_label_png(str(root / 'fix' / 'label' / f'{2 * k:05d}.png'), c['hair'])
        DS.write_label_png(str(root / 'fix' / 'label' / f'{2 * k + 1:05d}.png'), c['face'])
        lm[f'{2 * k:05d}'], lm[f'{2 * k + 1:05d}'] = c['hair_lm'], c['face_lm']
    pairs = [(('fix', f'{2 * k:05d}.png'), ('fix', f'{2 * k + 1:05d}.png')) for k in range(3)]
    warper = MaskWarper(device='cuda:0')
    done, skipped = DS.warp_pool(warper, str(root), str(tmp_path / 'pool'), lm, pairs, batch=2)
    assert len(done) == 3 and not skipped
    stack = lambda key: np.stack([c[key] for c in cs])
    ref = warper.warp_batch(stack('hair'), stack('face'), stack('hair_lm'), stack('face_lm'), mesher='device').cpu().numpy()
    assert int(warper.last_mesh_status.abs().sum()) == 0
    for k, name in enumerate(done):
        assert name == f'fix___{2 * k:05d}___fix___{2 * k + 1:05d}___00.png'
        assert np.array_equal(DS.read_gray(os.path.join(str(tmp_path / 'pool'), name)), ref[k])
