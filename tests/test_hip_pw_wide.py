"""GPU tests of option sean.pw_wide (exact-f32 path): the 64-row wave tiles of the 1x1 GEMM kernel (pw_conv_wide_kernel,
ctrlhair_amd/csrc/conv_pw.h) for the learned shortcuts and the grouped style-LUT launch, the transposed wave reduction of fc_mu
(sean_kernels.hip) and the one-thread-per-(row, label) F(4x4) style pack (conv_inst_wino4.hip).  Every output element is still one
v_mfma_f32_32x32x2_f32 accumulator chain over the same k-steps, every fc_mu sum the same additions commuted, every style-image value the
same expression: sean.pw_wide = 1 must give the bits of sean.pw_wide = 0.  Generator at ngf = 64:
  S = 64, B = 5: shortcuts 512 -> 256 at 16^2 (exactly one 256-pixel tile per sample), 256 -> 128 at 32^2, 128 -> 64 at 64^2; LUT launch of
                 95 (sample, label) rows = three row tiles: a half-empty row pair, the store mask and the skipped waves;
  S = 64, B = 9: 171 rows: three row pairs, a ragged last tile;
  S = 128, B = 2: shortcut 1024 -> 512 at 16^2 (four row groups); 38 rows take the <= 64-column route, which must not change."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 64


def _inputs(B, S):
    from ctrlhair_amd import procedural as P
    return P.blocky_labels(B, S, grid=8, seed=41), P.style_codes(B, seed=42), P.noise_planes(B, S, NGF, seed=43)


def _run(gen, lab, codes, noise, wide):
    gen.handle.set_option('sean.pw_wide', wide)
    dev = gen.device
    try:
        out = gen.generate(torch.from_numpy(lab).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        gen.handle.set_option('sean.pw_wide', 1)


@pytest.fixture(scope='module')
def gens(hip_lib):
    """One generator per (batch, size), shared by the cases of this module (sean.pw_wide may be set at any time)."""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    sd = P.sean_state_dict(0, NGF, calibrated=True)
    made = {}

    def get(B, S):
        if (B, S) not in made:
            made[(B, S)] = SeanGenerator(0, f16x3=0).load_state_dict(sd, max_batch=B, max_size=S)
        return made[(B, S)]
    yield get
    for g in made.values():
        g.handle.close()


@pytest.mark.parametrize('S,B', [(64, 5), (64, 9), (128, 2)])
def test_wide_tiles_give_the_same_bits(gens, S, B):
    lab, codes, noise = _inputs(B, S)
    gen = gens(B, S)
    old = _run(gen, lab, codes, noise, 0)
    assert np.isfinite(old).all()
    new = _run(gen, lab, codes, noise, 1)
    assert np.array_equal(old, new), float(np.abs(old - new).max())
    assert np.array_equal(new, _run(gen, lab, codes, noise, 1)), 'repeated call differs'


def test_a_smaller_call_after_a_larger_one(gens):
    """B = 5 after B = 9 on one handle against a handle that never ran the larger call: no row of the larger call may leak through the waves
    that skip their empty row tiles (the packed projections keep their pitch of the larger batch's last call only where it is rewritten)."""
    S = 64
    lab, codes, noise = _inputs(9, S)
    big = gens(9, S)
    full = _run(big, lab, codes, noise, 1)
    small = _run(big, lab[:5], codes[:5], noise[:5], 1)
    fresh = _run(gens(5, S), lab[:5], codes[:5], noise[:5], 1)
    assert np.array_equal(small, fresh), float(np.abs(small - fresh).max())
    assert np.array_equal(full, _run(big, lab, codes, noise, 1))
    assert np.array_equal(small, _run(big, lab[:5], codes[:5], noise[:5], 0))


def test_same_number_of_launches(gens):
    S, B = 64, 5
    lab, codes, noise = _inputs(B, S)
    gen = gens(B, S)
    n = {}
    for wide in (0, 1):
        gen.handle.profile_enable(True)
        try:
            _run(gen, lab, codes, noise, wide)
        finally:
            gen.handle.profile_enable(False)
        n[wide] = [gen.handle.profile_read(k)['launches'] for k in range(4)]
        gen.handle.profile_read(-1)
    print('launches per kind, pw_wide = 0 / 1:', n[0], n[1])
    assert n[0][0] > 0 and n[0][0] == n[1][0]
    assert n[0] == n[1]


def test_zencoder_phase_gemms(gens):
    """One Zencoder encode at S = 64, B = 2 with the option on and off.  The ConvTranspose's phase GEMMs call conv_pw with a sample stride
    (in_bs) and follow the same launcher rule; the library takes them from 16384 pixels per call on, so at this size the test pins that
    the option leaves the encoder's other routes alone (the large sizes: the pipeline leg's image comparison, profiles/r12_pw_wide.md)."""
    from ctrlhair_amd import procedural as P
    S, B = 64, 2
    gen = gens(5, S)
    lab, img = P.blocky_labels(B, S, grid=8, seed=44), P.synthetic_images(B, S, seed=45)
    out = {}
    for wide in (0, 1):
        gen.handle.set_option('sean.pw_wide', wide)
        try:
            c = gen.encode(torch.from_numpy(img).to(gen.device), torch.from_numpy(lab).to(gen.device))
            torch.cuda.synchronize()
            out[wide] = c.cpu().numpy()
        finally:
            gen.handle.set_option('sean.pw_wide', 1)
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0], out[1])
