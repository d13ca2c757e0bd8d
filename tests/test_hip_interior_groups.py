"""GPU tests of the channel-group loop of the four-pixel interior pass (ace_interior_f32_tile4_kernel, ctrlhair_amd/csrc/ace_sparse.hip;
option sean.int_groups): one block of 128 x 8 pixels sets up its marks, noise, ownership and the slots of its straight-edge codes once and
then serves several groups of 32 channels, with the table rows stored as {1 + gamma, beta} pairs.  Neither changes a single operation of
    out = act((bn_a x + nv nz + bn_d) (1 + gamma) + beta)          (normalization.py:111-112,182; architecture.py:95)
so every decomposition must give the same bits.  All cases run through SeanGenerator on the exact-f32 path with sean.edge at its default:
the levels of 128 pixels and more take the tile4 kernel with straight-edge marks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen(sd, mb, ms, extra=None):
    from ctrlhair_amd.sean.generator import SeanGenerator
    return SeanGenerator(0, f16x3=0, options=dict(extra or {})).load_state_dict(sd, max_batch=mb, max_size=ms)


def _run(gen, labels, codes, noise):
    dev = gen.device
    out = gen.generate(torch.from_numpy(labels).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run_groups(gen, groups, labels, codes, noise):
    gen.handle.set_option('sean.int_groups', groups)
    return _run(gen, labels, codes, noise)


def _label_sets(B, S):
    """The label sets of tests/test_hip_sparse_ace.py::_label_sets that the issue names (rebuilt here: that file stays as it is)."""
    from ctrlhair_amd import procedural as P
    sets = {}
    sets['blocky'] = P.blocky_labels(B, S, grid=8)
    sets['face'] = np.stack([P.face_like_labels(S, 40 + b) for b in range(B)])
    noclass = P.blocky_labels(B, S, grid=4, seed=77).copy()                    # labels >= 19 ("no class") never count as interior
    noclass[:, : S // 2, : S // 2] = 255
    noclass[:, S // 2:, S // 2:] = 19
    sets['noclass'] = noclass
    sets['one_region'] = np.full((B, S, S), 13, np.uint8)                      # everything interior except the image frame
    stripes = np.zeros((B, S, S), np.uint8)                                    # 5-pixel stripes: interior = exactly the centre line
    stripes[:] = ((np.arange(S) // 5) % 19)[None, None, :]
    sets['stripes5'] = stripes
    return sets


def _edge_codes(lab):
    """Straight-edge code of every pixel of one label map [H][W] (-1: none), from the definition in ace_sparse.h / ace_edge_code: the 5x5
    neighbourhood lies inside the image, is five uniform columns (orientation 0) or rows (1) A^s B^(5-s) with s = 1..4, A != B, both < 19;
    code = ((orientation * 19 + A) * 19 + B) * 4 + (s - 1).  Columns are tried first."""
    H, W = lab.shape
    out = np.full((H, W), -1, np.int32)
    L = lab.astype(np.int32)
    for y in range(2, H - 2):
        for x in range(2, W - 2):
            w = L[y - 2:y + 3, x - 2:x + 3]
            for o in (0, 1):
                v = w if o == 0 else w.T                   # v[i][j]: line j along the split direction
                if not (v == v[0:1, :]).all():
                    continue
                l = v[0]
                A, Bl = int(l[0]), int(l[4])
                if not (A < 19 and Bl < 19 and A != Bl):
                    continue
                s = 1
                for j in range(1, 4):
                    if l[j] == A and s == j:
                        s += 1
                if all(l[j] == (A if j < s else Bl) for j in range(1, 4)):
                    out[y, x] = ((o * 19 + A) * 19 + Bl) * 4 + (s - 1)
                    break
    return out


def _many_pairs_stripes(B, S):
    """Vertical stripes of 3 pixels whose ordered label pairs (left, right) never repeat along x: every border between two stripes gives the
    two codes (A, B, s = 3) and (A, B, s = 2) -- a window that sees a third stripe is no straight edge -- and no code occurs twice."""
    seq, used = [0], set()
    while len(seq) * 3 < S:
        a = seq[-1]
        nxt = next(b for k in range(1, 19) for b in [(a + k * 7) % 19] if (a, b) not in used)
        used.add((a, nxt))
        seq.append(nxt)
    row = np.repeat(np.asarray(seq, np.uint8), 3)[:S]
    lab = np.empty((B, S, S), np.uint8)
    for b in range(B):
        lab[b] = ((row.astype(np.int32) + 5 * b) % 19).astype(np.uint8)[None, :]      # another set of pairs per sample
    return lab


@pytest.mark.parametrize('ngf,S,B', [(64, 128, 3), (24, 160, 2)])
def test_channel_group_decompositions_are_bit_identical(hip_lib, ngf, S, B):
    """sean.int_groups = 1 (one group of 32 channels per block), 2 and 0 (the launcher's rule) on ngf = 64, S = 128, B = 3 (odd batch; 128 and 64
    channels at the 128-pixel level: 4 and 2 groups) and ngf = 24, S = 160, B = 2 (48 / 24 channels: a partial last group; W = 160: a ragged
    128-pixel tile): np.array_equal on every label set, and a repeated call at int_groups = 0 gives the same bits again (the block's table
    is filled through atomics, so its slot order may differ from run to run -- the values read from it may not)."""
    from ctrlhair_amd import procedural as P
    sd = P.sean_state_dict(0, ngf, calibrated=ngf in (16, 64))      # (the data file holds gains for ngf = 16 and 64 only; bit identity needs none)
    gen = _gen(sd, B, S)                                   # (one handle: the option may be set at any time)
    codes, noise = P.style_codes(B, seed=31), P.noise_planes(B, S, ngf, seed=32)
    for name, lab in _label_sets(B, S).items():
        ref = _run_groups(gen, 1, lab, codes, noise)
        assert np.isfinite(ref).all(), name
        for g in (2, 0):
            got = _run_groups(gen, g, lab, codes, noise)
            assert np.array_equal(ref, got), (name, g, float(np.abs(ref - got).max()))
        assert np.array_equal(ref, _run_groups(gen, 0, lab, codes, noise)), (name, 'repeated call differs')
    gen.handle.close()


def test_second_round_of_the_code_table(hip_lib):
    """More than 64 distinct straight-edge codes in one block of 128 x 8 pixels: the 64-slot table fills up and the block takes a second round
    (and, with several channel groups per block, the group loop inside each round).  3-pixel vertical stripes with ordered label pairs that
    never repeat along x give two codes per stripe border: about 80 per block at S = 128.  The codes are counted on the host from the
    definition in ace_sparse.h, so the test cannot pass without round two.  Same bits across int_groups 1 / 2 / 0, and <= 1e-5 against the
    boundary-conv evaluation (sean.edge = 0), the bound tests/test_hip_wino.py uses for edge rows on vs off."""
    from ctrlhair_amd import procedural as P
    ngf, S, B = 64, 128, 2
    lab = _many_pairs_stripes(B, S)
    per_block = []
    for b in range(B):
        ec = _edge_codes(lab[b][:16])                       # rows 8..15 are one block row (all rows of this map are equal)
        per_block.append(len(set(ec[8:16][ec[8:16] >= 0].tolist())))
    print('distinct straight-edge codes in a 128 x 8 block, per sample:', per_block)
    assert max(per_block) > 64
    sd = P.sean_state_dict(0, ngf)
    codes, noise = P.style_codes(B, seed=33), P.noise_planes(B, S, ngf, seed=34)
    gen = _gen(sd, B, S)
    ref = _run_groups(gen, 1, lab, codes, noise)
    assert np.isfinite(ref).all()
    for g in (2, 0):
        got = _run_groups(gen, g, lab, codes, noise)
        assert np.array_equal(ref, got), (g, float(np.abs(ref - got).max()))
    gen.handle.close()
    off = _gen(sd, B, S, {'sean.edge': 0})
    d = float(np.abs(ref - _run(off, lab, codes, noise)).max())
    print(f'second round: max |edge rows - boundary conv| = {d:.3e}')
    assert d <= 1e-5
    off.handle.close()


def test_group_loop_against_the_oracle(hip_lib):
    """One shape and one label set (face-like, first sample) at int_groups = 0 against the PyTorch oracle at the project's 1e-3."""
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    ngf, S = 64, 128
    sd = P.sean_state_dict(0, ngf)
    lab = P.face_like_labels(S, 40)[None]
    codes, noise = P.style_codes(1, seed=31), P.noise_planes(1, S, ngf, seed=32)
    gen = _gen(sd, 1, S, {'sean.int_groups': 0})
    got = _run(gen, lab, codes, noise)
    ref = O.generator_forward(O.to_torch(sd), lab, codes, noise, ngf).numpy()
    d = float(np.abs(got - ref).max())
    print(f'int_groups=0 ngf={ngf} S={S} face: max |hip - oracle| = {d:.3e}')
    assert d <= 1e-3
    gen.handle.close()
