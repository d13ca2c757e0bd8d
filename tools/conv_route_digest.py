"""SHA-256 of the outputs of a fixed list of calls, and the kind-0 (plain conv) profile record of a few of them, as JSON.

    python tools/conv_route_digest.py OUT.json

Two builds that route every plain conv alike and launch it with the same arguments give the same file: the digests cover the
bytes of every output, the kind-0 record (launches, dense FLOPs, executed FLOPs, bytes -- the executed FLOPs differ per route)
fingerprints the routes.  Calls: the SEAN generator on its four paths (ngf 16, S in {64, 128, 256}, B in {1, 3} on a handle with
max_batch = 2, so B = 3 runs in two chunks), the exact-f32 path also under sean.wino 0 / 1, sean.wino4_force and sean.batch_invariant;
the Zencoder's feature map (tap zenc.feat: the codes are region means accumulated with float atomics) on both paths at S in
{64, 96, 256, 288} and with sean.convt_gemm = 0; the shape encoder / decoder and BiSeNet on both paths and with aux.wino = 0.
Every entry is computed twice; an entry whose two runs differ is listed under "unstable" with their maximum absolute difference.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ctrlhair_amd import lib, models                     # noqa: E402
from ctrlhair_amd import procedural as P                 # noqa: E402
from ctrlhair_amd.sean.generator import SeanGenerator    # noqa: E402

NGF = 16
PATHS = {'f32': 0, 'f16x3': 1, 'f16': 2, 'bf16': 3}       # option sean.f16x3
digests, unstable, records = {}, {}, {}


def put(name, fn):
    """fn() -> dict of arrays; run twice, digest the first, note run-to-run differences"""
    a, b = fn(), fn()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        digests[f'{name}/{k}'] = hashlib.sha256(x.tobytes()).hexdigest()
        if not np.array_equal(x, y):
            unstable[f'{name}/{k}'] = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max())


def generator_calls(tag, path, options, sizes=(64, 128, 256), batches=(1, 3), record=False):
    g = make_gen(path, options)
    for S in sizes:
        for B in batches:
            lab = torch.from_numpy(P.blocky_labels(B, S, grid=8, seed=100 + S)).to(g.device)
            codes = torch.from_numpy(P.style_codes(B, seed=200 + S)).to(g.device)
            noise = torch.from_numpy(P.noise_planes(B, S, NGF, seed=300 + S)).to(g.device)

            def run():
                out = g.generate(lab, codes, noise)
                torch.cuda.synchronize()
                return {'image': out.cpu().numpy()}
            put(f'gen/{tag}/S{S}_B{B}', run)
    if record:
        B, S = 2, 256
        lab = torch.from_numpy(P.blocky_labels(B, S, grid=8, seed=400)).to(g.device)
        codes = torch.from_numpy(P.style_codes(B, seed=401)).to(g.device)
        noise = torch.from_numpy(P.noise_planes(B, S, NGF, seed=402)).to(g.device)
        g.handle.profile_enable(True)
        g.generate(lab, codes, noise)
        torch.cuda.synchronize()
        r = g.handle.profile_read(0)
        g.handle.profile_enable(False)
        records[f'gen/{tag}/S{S}_B{B}'] = {k: r[k] for k in ('launches', 'flops', 'flops_executed', 'bytes')}
    g.handle.close()


def make_gen(path, options, max_size=256):
    return SeanGenerator(0, f16x3=PATHS[path], options=options).load_state_dict(SD, max_batch=2, max_size=max_size)


def zencoder_calls(tag, path, options, max_batch=2, sizes=(64, 96, 256, 288)):
    """max_batch = 4 at S = 256: 16384 quarter-resolution pixels per chunk, where the ConvTranspose takes its phase GEMMs"""
    g = SeanGenerator(0, f16x3=PATHS[path], options=options).load_state_dict(SD, max_batch=max_batch, max_size=max(sizes))
    for S in sizes:
        B = max_batch + 1
        lab = torch.from_numpy(P.blocky_labels(B, S, grid=8, seed=500 + S)).to(g.device)
        img = torch.from_numpy(P.synthetic_images(B, S, seed=600 + S)).to(g.device)

        def run():
            feat = torch.zeros(max_batch, 512, S // 2, S // 2, device=g.device)
            g.handle.sean_set_tap('zenc.feat', feat.data_ptr())
            g.encode(img, lab)
            torch.cuda.synchronize()
            g.handle.sean_set_tap('zenc.feat', None)
            return {'feat_last_chunk': feat[:1].cpu().numpy()}
        put(f'zenc/{tag}/S{S}_B{B}', run)
        for Bc in (max_batch,):       # one whole chunk: every sample of the tap
            def run2():
                feat = torch.zeros(max_batch, 512, S // 2, S // 2, device=g.device)
                g.handle.sean_set_tap('zenc.feat', feat.data_ptr())
                g.encode(img[:Bc], lab[:Bc])
                torch.cuda.synchronize()
                g.handle.sean_set_tap('zenc.feat', None)
                return {'feat': feat.cpu().numpy()}
            put(f'zenc/{tag}/S{S}_B{Bc}', run2)
    g.handle.close()


def aux_calls(tag, f16x3, wino):
    dev = torch.device('cuda', 0)
    h = lib.Handle(0)
    h.set_option('aux.wino', wino)
    sg = models.ShapeGenerator(h, dev).load_state_dict(P.shape_state_dict(0), max_batch=2, f16x3=f16x3)
    fp = models.FaceParsing(h, dev).load_state_dict(P.bisenet_state_dict(0), max_batch=2, max_size=512, f16x3=f16x3)
    lab = torch.from_numpy(np.stack([P.face_like_labels(256, 700 + b) for b in range(3)])).to(dev)

    def shape():
        hair, face = sg.encode_labels(lab)
        hl, fl, lb, pr = sg._decode(hair, face, want_hair=True, want_face=True, want_labels=True)
        torch.cuda.synchronize()
        return {'hair_code': hair.cpu().numpy(), 'face_code': face.cpu().numpy(), 'hair_logit': hl.cpu().numpy(),
                'face_logit': fl.cpu().numpy(), 'labels': lb.cpu().numpy()}
    put(f'shape/{tag}', shape)
    for S in (256, 512):
        img = torch.from_numpy(P.synthetic_images(3, S, seed=800 + S)).to(dev)

        def parse():
            lb, lg = fp.parse_tensor(img, want_logits=True)
            torch.cuda.synchronize()
            return {'labels': lb.cpu().numpy(), 'logits': lg.cpu().numpy()}
        put(f'bisenet/{tag}/S{S}', parse)
    h.close()


def main():
    global SD
    out = sys.argv[1] if len(sys.argv) > 1 else 'conv_route_digest.json'
    SD = P.sean_state_dict(0, NGF)
    for path in PATHS:
        generator_calls(path, path, {}, record=True)
    for tag, options in (('f32_wino0', {'sean.wino': 0}), ('f32_wino1', {'sean.wino': 1}), ('f32_wino4_force', {'sean.wino4_force': 1}),
                         ('f32_batch_invariant', {'sean.batch_invariant': 1})):
        generator_calls(tag, 'f32', options)
    for path in ('f32', 'f16x3'):
        zencoder_calls(path, path, {})
    zencoder_calls('f32_convt_gemm0', 'f32', {'sean.convt_gemm': 0})
    zencoder_calls('f32_mb4', 'f32', {}, max_batch=4, sizes=(256,))
    zencoder_calls('f32_mb4_convt_gemm0', 'f32', {'sean.convt_gemm': 0}, max_batch=4, sizes=(256,))
    for f16x3 in (False, True):
        aux_calls('f16x3' if f16x3 else 'f32', f16x3, 1)
    aux_calls('f32_wino0', False, 0)
    res = {'digests': digests, 'unstable_max_abs_diff': unstable, 'profile_kind0': records}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'entries': len(digests), 'unstable': unstable, 'profile_kind0': records}))


if __name__ == '__main__':
    main()
