"""Status codes and messages of the C ABI's host-side argument checks, as one JSON table.

    python tools/abi_error_digest.py OUT.json

Every ch_* entry point that takes a handle is called with arguments it refuses BEFORE any launch (a null handle, a null pointer, N = 0,
a channel count of 2, a workspace one byte short of its query, a non-finite plan value, a misaligned workspace, a distance of 1, a
model that was never finalized ...), and every size query with arguments outside its range.  Each call becomes one record
{entry, case, status, message}: for an entry point its status code and ch_last_error, for a query the value it returned (message '').
No case hands a bad pointer or size to a kernel and none can produce a HIP error: the pointers that are not null point into one
zero-filled device buffer and are never read, because the call returns first.

tests/golden/abi_errors.json is this table recorded before the entry points' common tail moved into launch() / workspace_short()
(csrc/ch_api.cpp); tests/test_hip_abi_messages.py replays collect() against it.  Needs a GPU only because ch_create does.
"""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BUF_BYTES = 4 << 20
NO_MESSAGE = ('ch_sean_set_tap', 'ch_profile_enable')      # with a handle these refuse without a message, or not at all
# Entry points added after the table was recorded.  The table is a snapshot that guards the messages of the entry points it holds; a
# later entry point's refusals and messages are asserted where it is tested (ch_jpeg_decode: tests/test_hip_jpegdec.py::test_abi_refusals,
# ch_jpeg_decode_rst: tests/test_hip_jpegdec_rst.py::test_abi_refusals, ch_ingest_*: tests/test_hip_ingest.py::test_abi_refusals,
# ch_sean_code_memo_stats: a query, its counters are asserted call by call in tests/test_hip_code_memo.py,
# ch_orient_*: tests/test_hip_orient.py::test_abi_refusals)
AFTER_THE_TABLE = ('ch_jpeg_decode', 'ch_jpeg_decode_rst', 'ch_ingest_workspace_bytes', 'ch_ingest_images', 'ch_ingest_labels',
                   'ch_sean_code_memo_stats', 'ch_orient_workspace_bytes', 'ch_orient_u8')


def handle_entries(symbols):
    """Names of the entry points whose first argument is the handle (those of the recorded table: not AFTER_THE_TABLE)."""
    return sorted(n for n, (res, args) in symbols.items()
                  if n not in AFTER_THE_TABLE and ((res is C.c_int and args[:1] == [C.c_void_p]) or n == 'ch_sean_noise_floats'))


def _zero(argtype):
    return 0.0 if argtype is C.c_double else (0 if argtype in (C.c_int, C.c_uint64, C.c_size_t) else None)


def collect():
    """The records, in table order (a list of dicts)."""
    import numpy as np
    import torch
    from ctrlhair_amd import lib as L

    h = L.Handle(0)
    lib = h.lib
    buf = torch.zeros(BUF_BYTES, dtype=torch.uint8, device='cuda:0')
    p = buf.data_ptr()
    assert p % 256 == 0
    q = p + (BUF_BYTES >> 1)                                  # a second region, far from the first
    records = []

    def call(entry, case, *args):
        rc = int(getattr(lib, entry)(h._h, *args))
        records.append({'entry': entry, 'case': case, 'status': rc, 'message': lib.ch_last_error(h._h).decode() if rc else ''})

    def query(entry, case, *args):
        records.append({'entry': entry, 'case': case, 'status': int(getattr(lib, entry)(*args)), 'message': ''})

    def need_of(entry, *args):
        need = int(getattr(lib, entry)(*args))
        assert 0 < need <= BUF_BYTES >> 1 or entry in ('ch_mask_warp_workspace_bytes', 'ch_delaunay_workspace_bytes'), (entry, need)
        return need

    def f64(values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        return a, a.ctypes.data_as(C.c_void_p)

    def i32(values):
        a = np.ascontiguousarray(values, dtype=np.int32)
        return a, a.ctypes.data_as(C.c_void_p)

    # ---- a null handle, every entry ------------------------------------------------------------------------------------------------
    for entry in handle_entries(L.SYMBOLS):
        args = [_zero(t) for t in L.SYMBOLS[entry][1][1:]]
        rc = int(getattr(lib, entry)(None, *args))
        records.append({'entry': entry, 'case': 'null handle', 'status': rc, 'message': lib.ch_last_error(None).decode()})

    # ---- weights, options, state ---------------------------------------------------------------------------------------------------
    host = np.zeros(4, np.float32)
    hp = host.ctypes.data_as(C.c_void_p)
    shape = (C.c_int64 * 1)(4)
    call('ch_load_tensor', 'null name', 0, None, hp, L.F32, shape, 1)
    call('ch_load_tensor', 'ndim 9', 0, b'w', hp, L.F32, shape, 9)
    call('ch_load_tensor', 'model 9', 9, b'w', hp, L.F32, shape, 1)
    call('ch_load_tensor', 'dtype 5', 0, b'w', hp, 5, shape, 1)
    call('ch_load_tensor', 'negative dimension', 0, b'w', hp, L.F32, (C.c_int64 * 1)(-1), 1)
    call('ch_set_option', 'unknown option', b'no.such.option', 1)
    call('ch_finalize', 'model 7', 7, 1, 64)
    call('ch_finalize', 'model -1', -1, 1, 64)
    records.append({'entry': 'ch_sean_noise_floats', 'case': 'not finalized', 'status': int(lib.ch_sean_noise_floats(h._h, 64)), 'message': ''})
    call('ch_sean_generate', 'not finalized', p, p, None, 0, p, 1, 64, None)
    call('ch_sean_draw_noise', 'not finalized', 0, p, 1, 64, None)
    call('ch_sean_encode', 'not finalized', p, p, p, 1, 64, None)
    call('ch_sean_encode_features', 'not finalized', p, 1, 64, None)
    call('ch_sean_encode_regions', 'not finalized', p, p, 1, 64, None)
    call('ch_sean_scale_report', 'not finalized', (C.c_float * 36)(), 36)
    call('ch_sean_debug_read', 'not finalized', hp, 16)
    call('ch_profile_read', 'no records', -1, None, None, None, None)
    call('ch_profile_read_ex', 'no records', -1, None, None, None, None, None)
    call('ch_mfma_peak', 'kind 2', 2, 30, C.byref(C.c_double()))
    call('ch_mfma_peak', 'ms_target 0', 0, 0, C.byref(C.c_double()))
    call('ch_mfma_peak', 'null result', 0, 30, None)

    # ---- the small models: argument checks, then the model's own refusal (never finalized) -------------------------------------------
    call('ch_color_generate', 'null cond', p, None, p, 1, None)
    call('ch_color_generate', 'B 0', p, p, p, 0, None)
    call('ch_color_generate', 'not finalized', p, p, p, 1, None)
    call('ch_color_encode', 'null out', p, None, 1, None)
    call('ch_color_encode', 'not finalized', p, p, 1, None)
    call('ch_color_predict', 'B 0', p, p, 0, None)
    call('ch_color_predict', 'not finalized', p, p, 1, None)
    call('ch_shape_encode', 'neither code', p, None, None, 1, None)
    call('ch_shape_encode', 'not finalized', p, p, p, 1, None)
    call('ch_shape_decode', 'labels without hair_code', None, p, None, None, p, None, 1, None)
    call('ch_shape_decode', 'not finalized', p, p, None, None, p, None, 1, None)
    call('ch_shape_combine', 'null labels', p, p, None, None, 1, None)
    call('ch_shape_combine', 'not finalized', p, p, p, None, 1, None)
    call('ch_bisenet_parse', 'null labels', p, None, None, 1, 64, 64, None)
    call('ch_bisenet_parse', 'not finalized', p, p, None, 1, 64, 64, None)

    # ---- blending ------------------------------------------------------------------------------------------------------------------
    call('ch_blend_mask', 'null target_parsing', None, p, p, 8, 8, None)
    call('ch_blend_mask', 'H 0', p, p, p, 0, 8, None)
    call('ch_blend_mask_batch', 'B 0', p, p, p, 0, 8, 8, None)
    call('ch_blend_mask_batch', 'B 65536', p, p, p, 65536, 8, 8, None)
    call('ch_poisson_blend', 'H 2', p, p, p, p, 2, 2, 1, 10, 1e-7, None, None)
    call('ch_poisson_blend', 'rel_tol nan', p, p, p, p, 8, 8, 1, 10, math.nan, None, None)
    call('ch_poisson_blend_batch', 'B 0', p, p, p, p, 0, 8, 8, 1, 10, 1e-7, None, None)
    call('ch_poisson_blend_batch', 'max_iters -1', p, p, p, p, 1, 8, 8, 1, -1, 1e-7, None, None)

    # ---- mask warp and meshing -------------------------------------------------------------------------------------------------------
    for B in (0, -1):
        query('ch_mask_warp_workspace_bytes', f'B {B}', B)
        query('ch_delaunay_workspace_bytes', f'B {B}', B)
    wneed = need_of('ch_mask_warp_workspace_bytes', 1)
    good_desc, good_dp = i32([0, 3, 0, 1, 0, 0])
    for entry in ('ch_mask_warp_batch', 'ch_mask_warp_batch_dev'):
        call(entry, 'null V', p, p, None, p, p, p, good_dp, None, p, None, None, p, wneed, 1, None)
        call(entry, 'no constraints and no U_in', p, p, p, p, None, None, good_dp, None, p, None, None, p, wneed, 1, None)
        call(entry, 'B 0', p, p, p, p, p, p, good_dp, None, p, None, None, p, wneed, 0, None)
        call(entry, 'workspace one byte short', p, p, p, p, p, p, good_dp, None, p, None, None, p, wneed - 1, 1, None)
    _, dp = i32([-1, 3, 0, 1, 0, 0])
    call('ch_mask_warp_batch', 'negative offset in desc', p, p, p, p, p, p, dp, None, p, None, None, p, wneed, 1, None)
    _, dp = i32([0, 2, 0, 1, 0, 0])
    call('ch_mask_warp_batch', 'two vertices', p, p, p, p, p, p, dp, None, p, None, None, p, wneed, 1, None)
    _, dp = i32([0, 3, 0, 4097, 0, 0])
    call('ch_mask_warp_batch', '4097 triangles', p, p, p, p, p, p, dp, None, p, None, None, p, wneed, 1, None)
    dneed = need_of('ch_delaunay_workspace_bytes', 1)
    _, vd = i32([0, 3])
    call('ch_delaunay_batch', 'null status', p, vd, p, p, None, p, dneed, 1, None)
    call('ch_delaunay_batch', 'B 0', p, vd, p, p, p, p, dneed, 0, None)
    call('ch_delaunay_batch', 'workspace one byte short', p, vd, p, p, p, p, dneed - 1, 1, None)
    _, bad_vd = i32([-4, 3])
    call('ch_delaunay_batch', 'negative offset in v_desc', p, bad_vd, p, p, p, p, dneed, 1, None)

    # ---- face alignment ------------------------------------------------------------------------------------------------------------------
    query('ch_resample_lanczos_workspace_bytes', 'C 5', 16, 16, 5, 8, 8)
    query('ch_resample_lanczos_workspace_bytes', 'Hs 0', 0, 16, 3, 8, 8)
    query('ch_resample_lanczos_workspace_bytes', 'Wd 32769', 16, 16, 3, 8, 32769)
    lneed = need_of('ch_resample_lanczos_workspace_bytes', 16, 16, 3, 8, 8)
    call('ch_resample_lanczos_u8', 'null dst', p, 16, 16, 3, None, 8, 8, q, lneed, None)
    call('ch_resample_lanczos_u8', 'C 5', p, 16, 16, 5, p, 8, 8, q, lneed, None)
    call('ch_resample_lanczos_u8', 'Hs 0', p, 0, 16, 3, p, 8, 8, q, lneed, None)
    call('ch_resample_lanczos_u8', 'workspace one byte short', p, 16, 16, 3, p, 8, 8, q, lneed - 1, None)
    query('ch_quad_warp_workspace_bytes', 'T below S', 4, 8)
    query('ch_quad_warp_workspace_bytes', 'T 16385', 16385, 8)
    query('ch_quad_warp_workspace_bytes', 'S 0', 8, 0)
    qneed = need_of('ch_quad_warp_workspace_bytes', 8, 4)
    _, coef = f64([1, 0, 0, 0, 1, 0, 0, 0])
    call('ch_quad_warp_resample_u8', 'T below S', p, 16, 16, coef, 4, 8, p, q, qneed, None)
    call('ch_quad_warp_resample_u8', 'null workspace with S below T', p, 16, 16, coef, 8, 4, p, None, qneed, None)
    _, bad_coef = f64([1, 0, 0, 0, math.inf, 0, 0, 0])
    call('ch_quad_warp_resample_u8', 'coefficient not finite', p, 16, 16, bad_coef, 8, 4, p, q, qneed, None)
    call('ch_quad_warp_resample_u8', 'workspace one byte short', p, 16, 16, coef, 8, 4, p, q, qneed - 1, None)
    _, pads = i32([1, 1, 1, 1])
    _, zero_pads = i32([1, 0, 1, 1])
    _, gauss = f64([1.0])
    query('ch_align_pad_workspace_bytes', 'null pads', 16, 16, None, 0)
    query('ch_align_pad_workspace_bytes', 'pad 0', 16, 16, zero_pads, 0)
    query('ch_align_pad_workspace_bytes', 'radius -1', 16, 16, pads, -1)
    query('ch_align_pad_workspace_bytes', 'padded size out of range', 32768, 16, pads, 0)
    pneed = need_of('ch_align_pad_workspace_bytes', 16, 16, pads, 0)
    call('ch_align_pad_feather_u8', 'pad 0', p, 16, 16, zero_pads, gauss, 0, p, q, pneed, None)
    call('ch_align_pad_feather_u8', 'null gauss_w', p, 16, 16, pads, None, 0, p, q, pneed, None)
    call('ch_align_pad_feather_u8', 'padded size out of range', p, 32768, 16, pads, gauss, 0, p, q, pneed, None)
    call('ch_align_pad_feather_u8', 'workspace one byte short', p, 16, 16, pads, gauss, 0, p, q, pneed - 1, None)

    def align_plan(**change):
        """A plan that fits a 16 x 16 photo: no shrink, the whole photo as crop box, no padding, T = S = 8."""
        d = [0.0] * 24
        d[0], d[1], d[2] = 1, 16, 16
        d[3], d[4], d[5], d[6] = 0, 0, 16, 16
        d[12:20] = [0, 0, 0, 16, 16, 16, 16, 0]
        d[20], d[21] = 8, 8
        for k, v in change.items():
            d[int(k[1:])] = v
        return f64(d)

    _, plan = align_plan()
    query('ch_face_align_workspace_bytes', 'null plan', 16, 16, None, 0)
    query('ch_face_align_workspace_bytes', 'radius -1', 16, 16, plan, -1)
    query('ch_face_align_workspace_bytes', 'plan not finite', 16, 16, align_plan(d12=math.nan)[1], 0)
    query('ch_face_align_workspace_bytes', 'H 0', 0, 16, plan, 0)
    aneed = need_of('ch_face_align_workspace_bytes', 16, 16, plan, 0)
    call('ch_face_align', 'null plan', p, 16, 16, None, None, 0, p, q, aneed, None)
    call('ch_face_align', 'W 32769', p, 16, 32769, plan, None, 0, p, q, aneed, None)
    for case, change in (('plan[12] not finite', {'d12': math.nan}), ('plan[3] not an integer', {'d3': 0.5}),
                         ('output_size not an integer', {'d21': 7.5}), ('negative shrink', {'d0': -1}),
                         ('resized size without a shrink', {'d1': 15}), ('resized size out of range', {'d0': 2, 'd1': 0}),
                         ('resized size not the divided one', {'d0': 2, 'd1': 7, 'd2': 8}), ('crop box outside', {'d5': 17}),
                         ('pad 0', {'d7': 1, 'd8': 0, 'd9': 1, 'd10': 1, 'd11': 1}),
                         ('padded size out of range', {'d7': 1, 'd8': 32768, 'd9': 1, 'd10': 1, 'd11': 1}),
                         ('output_size above transform_size', {'d20': 4}), ('transform_size 16385', {'d20': 16385})):
        call('ch_face_align', case, p, 16, 16, align_plan(**change)[1], None, 0, p, q, aneed, None)
    padded = align_plan(d7=1, d8=1, d9=1, d10=1, d11=1)[1]
    call('ch_face_align', 'the plan pads and gauss_w is null', p, 16, 16, padded, None, 0, p, q, BUF_BYTES >> 1, None)
    call('ch_face_align', 'workspace one byte short', p, 16, 16, plan, None, 0, p, q, aneed - 1, None)

    # ---- paste-back --------------------------------------------------------------------------------------------------------------------------
    def unalign_plan(**change):
        """A plan that fits a 16 x 16 photo: the identity map, bbox (0, 0)-(8, 8), scale 1, S = 8."""
        d = [0.0] * 16
        d[0], d[4] = 1, 1
        d[6], d[7], d[8], d[9] = 0, 0, 8, 8
        d[10], d[11] = 1, 8
        for k, v in change.items():
            d[int(k[1:])] = v
        return f64(d)

    _, uplan = unalign_plan()
    bad_plans = (('plan[2] not finite', {'d2': math.inf}), ('plan[6] not an integer', {'d6': 0.5}), ('bbox outside the photo', {'d8': 17}),
                 ('bbox empty', {'d8': 0}), ('scale 0', {'d10': 0}), ('scale 17', {'d10': 17}), ('output_size 0', {'d11': 0}),
                 ('output_size 16385', {'d11': 16385}))
    call('ch_face_unalign', 'null edits', p, 16, 16, None, 1, None, uplan, 0.5, q, None)
    call('ch_face_unalign', 'N 0', p, 16, 16, q, 0, None, uplan, 0.5, q, None)
    call('ch_face_unalign', 'feather not finite', p, 16, 16, q, 1, None, uplan, math.nan, q, None)
    for case, change in bad_plans:
        call('ch_face_unalign', case, p, 16, 16, q, 1, None, unalign_plan(**change)[1], 0.5, q, None)
    call('ch_face_unalign', 'out overlaps photo', p, 16, 16, q, 1, None, uplan, 0.5, p + 16, None)
    query('ch_face_unalign_matte_workspace_bytes', 'null plan', 16, 16, None, 4)
    query('ch_face_unalign_matte_workspace_bytes', 'radius 0', 16, 16, uplan, 0)
    query('ch_face_unalign_matte_workspace_bytes', 'radius 65', 16, 16, uplan, 65)
    query('ch_face_unalign_matte_workspace_bytes', 'bbox not finite', 16, 16, unalign_plan(d7=math.nan)[1], 4)
    query('ch_face_unalign_matte_workspace_bytes', 'bbox outside the photo', 16, 16, unalign_plan(d9=17)[1], 4)
    mneed = need_of('ch_face_unalign_matte_workspace_bytes', 16, 16, uplan, 4)
    ws, out, edits, alpha = q, p + 4096, p + 8192, p + 16384        # photo: p .. p + 768

    def matte(case, plan_ptr=uplan, weight=p + 12288, radius=4, eps=1e-4, ws=ws, ws_bytes=mneed, alpha=alpha, N=1):
        call('ch_face_unalign_matte', case, p, 16, 16, edits, N, weight, plan_ptr, 0.5, radius, eps, out, alpha, ws, ws_bytes, None)

    matte('N 65536', N=65536)
    for case, change in bad_plans[:3]:
        matte(case, plan_ptr=unalign_plan(**change)[1])
    matte('null weight', weight=None)
    matte('radius 0', radius=0)
    matte('radius 65', radius=65)
    matte('eps 0', eps=0.0)
    matte('eps not finite', eps=math.inf)
    matte('null workspace', ws=None)
    matte('workspace misaligned', ws=ws + 16)
    matte('workspace one byte short', ws_bytes=mneed - 1)
    matte('alpha_out misaligned', alpha=alpha + 2)

    # ---- median style codes ----------------------------------------------------------------------------------------------------------------
    off = np.array([0, 4], np.int64)
    op = off.ctypes.data_as(C.c_void_p)
    descending = np.array([0, 4, 2], np.int64).ctypes.data_as(C.c_void_p)
    query('ch_style_medoid_workspace_bytes', 'null seg_offsets', None, 1, 8, 0)
    query('ch_style_medoid_workspace_bytes', 'dim 6', op, 1, 6, 0)
    query('ch_style_medoid_workspace_bytes', 'R 0', op, 0, 8, 0)
    query('ch_style_medoid_workspace_bytes', 'descending seg_offsets', descending, 2, 8, 0)
    sneed = need_of('ch_style_medoid_workspace_bytes', op, 1, 8, 0)
    call('ch_style_medoid', 'dim 6', p, op, 1, 6, 0, p, None, p, q, sneed, None)
    call('ch_style_medoid', 'n_split -1', p, op, 1, 8, -1, p, None, p, q, sneed, None)
    call('ch_style_medoid', 'null index', p, op, 1, 8, 0, None, None, p, q, sneed, None)
    call('ch_style_medoid', 'codes misaligned', p + 4, op, 1, 8, 0, p, None, p, q, sneed, None)
    call('ch_style_medoid', 'workspace one byte short', p, op, 1, 8, 0, p, None, p, q, sneed - 1, None)

    # ---- colour statistics, contact sheets, sweep statistics ---------------------------------------------------------------------------------
    call('ch_resize_linear_u8', 'C 5', p, q, 1, 8, 8, 5, 4, 4, None)
    call('ch_resize_linear_u8', 'B 0', p, q, 0, 8, 8, 3, 4, 4, None)
    call('ch_resize_linear_u8', 'Hd 65536', p, q, 1, 8, 8, 3, 65536, 4, None)
    call('ch_hair_erode', 'label 256', p, 1, 8, 8, 256, 19, q, 8, 8, None)
    call('ch_hair_erode', 'ksize even', p, 1, 8, 8, 13, 18, q, 8, 8, None)
    call('ch_hair_erode', 'ksize 33', p, 1, 8, 8, 13, 33, q, 8, 8, None)
    call('ch_hair_color_stats', 'null sums', p, p, 1, 8, 8, None, None)
    call('ch_hair_color_stats', 'H * W too large', p, p, 1, 50000, 50000, q, None)
    call('ch_sheet_compose', 'kind 3', p, 3, 1, 8, 8, p, None, q, 1, 1, 8, 8, 0, None)
    call('ch_sheet_compose', 'labels without lut', p, 2, 1, 8, 8, p, None, q, 1, 1, 8, 8, 0, None)
    call('ch_sheet_compose', 'n 0', p, 1, 0, 8, 8, p, None, q, 1, 1, 8, 8, 0, None)
    call('ch_sheet_compose', 'margin -1', p, 1, 1, 8, 8, p, None, q, 1, 1, 8, 8, -1, None)
    call('ch_sheet_compose', 'sheet too large', p, 1, 1, 8, 8, p, None, q, 70000, 1, 70000, 8, 0, None)
    call('ch_sweep_stats', 'kind 2', p, 2, p, p, 1, 8, 8, 8, 8, q, None)
    call('ch_sweep_stats', 'N 0', p, 1, p, p, 0, 8, 8, 8, 8, q, None)
    call('ch_sweep_stats', 'lh 0', p, 1, p, p, 1, 8, 8, 0, 8, q, None)
    call('ch_sweep_stats', 'H 40000', p, 1, p, p, 1, 40000, 8, 8, 8, q, None)

    # ---- PNG and JPEG ----------------------------------------------------------------------------------------------------------------------
    query('ch_png_zlib_bound', 'C 2', 8, 8, 2)
    query('ch_png_zlib_bound', 'H 0', 0, 8, 3)
    query('ch_png_zlib_bound', 'W 32769', 8, 32769, 3)
    for entry in ('ch_png_encode_workspace_bytes', 'ch_png_decode_workspace_bytes'):
        query(entry, 'N 0', 0, 8, 8, 3)
        query(entry, 'N 65536', 65536, 8, 8, 3)
        query(entry, 'C 2', 1, 8, 8, 2)
        query(entry, 'H 32769', 1, 32769, 8, 3)
    eneed = need_of('ch_png_encode_workspace_bytes', 1, 8, 8, 3)

    def png(entry, case, img=p, N=1, H=8, W=8, Cn=3, filt=-1, dist=None, ndist=0, sizes=p + 4096, ws=q, ws_bytes=eneed):
        extra = () if entry == 'ch_png_encode' else (dist, ndist)
        call(entry, case, img, N, H, W, Cn, filt, *extra, p + 8192, sizes, ws, ws_bytes, None)

    for entry in ('ch_png_encode', 'ch_png_encode_dist'):
        png(entry, 'null img', img=None)
        png(entry, 'null sizes', sizes=None)
        png(entry, 'C 2', Cn=2)
        png(entry, 'filter 5', filt=5)
        png(entry, 'N 0', N=0)
        png(entry, 'H 0', H=0)
        png(entry, 'workspace misaligned', ws=q + 8)
        png(entry, 'workspace one byte short', ws_bytes=eneed - 1)
    ints = lambda *v: (C.c_int * len(v))(*v)
    png('ch_png_encode_dist', 'ndist 4', dist=ints(2, 3, 4, 5), ndist=4)
    png('ch_png_encode_dist', 'null dist with ndist 1', ndist=1)
    png('ch_png_encode_dist', 'distance 1', dist=ints(1), ndist=1)
    png('ch_png_encode_dist', 'distance 32768', dist=ints(24, 32768), ndist=2)
    png('ch_png_encode_dist', 'duplicate distance', dist=ints(24, 24), ndist=2)
    dec_need = need_of('ch_png_decode_workspace_bytes', 1, 8, 8, 3)
    call('ch_png_decode', 'null offsets', p + 64, None, 1, 8, 8, 3, p + 8192, p + 4096, q, dec_need, None)
    call('ch_png_decode', 'N 0', p + 64, p, 0, 8, 8, 3, p + 8192, p + 4096, q, dec_need, None)
    call('ch_png_decode', 'C 2', p + 64, p, 1, 8, 8, 2, p + 8192, p + 4096, q, dec_need, None)
    call('ch_png_decode', 'workspace misaligned', p + 64, p, 1, 8, 8, 3, p + 8192, p + 4096, q + 8, dec_need, None)
    call('ch_png_decode', 'workspace one byte short', p + 64, p, 1, 8, 8, 3, p + 8192, p + 4096, q, dec_need - 1, None)
    query('ch_jpeg_scan_bound', 'C 4', 8, 8, 4, 2)
    query('ch_jpeg_scan_bound', 'subsampling 1', 8, 8, 3, 1)
    query('ch_jpeg_scan_bound', 'W 0', 8, 0, 3, 2)
    query('ch_jpeg_encode_workspace_bytes', 'N 0', 0, 8, 8, 3, 2)
    query('ch_jpeg_encode_workspace_bytes', 'N 65536', 65536, 8, 8, 3, 2)
    query('ch_jpeg_encode_workspace_bytes', 'C 2', 1, 8, 8, 2, 2)
    jneed = need_of('ch_jpeg_encode_workspace_bytes', 1, 8, 8, 3, 2)

    def jpeg(case, img=p, N=1, H=8, W=8, Cn=3, quality=75, sub=2, ws=q, ws_bytes=jneed):
        call('ch_jpeg_encode', case, img, N, H, W, Cn, quality, sub, p + 8192, p + 4096, ws, ws_bytes, None)

    jpeg('null img', img=None)
    jpeg('C 4', Cn=4)
    jpeg('quality 0', quality=0)
    jpeg('quality 101', quality=101)
    jpeg('subsampling 1', sub=1)
    jpeg('N 0', N=0)
    jpeg('W 32769', W=32769)
    jpeg('workspace misaligned', ws=q + 8)
    jpeg('workspace one byte short', ws_bytes=jneed - 1)

    torch.cuda.synchronize()                     # nothing was launched: this only shows that the device is as it was
    h.close()
    covered = {r['entry'] for r in records if r['case'] != 'null handle'}
    missing = [e for e in handle_entries(L.SYMBOLS) if e not in covered and e not in NO_MESSAGE]
    assert not missing, f'entry points without a case: {missing}'
    return records


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    records = collect()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(records, f, indent=1)
        f.write('\n')
    print(f'{len(records)} records, {len({r["entry"] for r in records})} entry points -> {sys.argv[1]}')


if __name__ == '__main__':
    main()
