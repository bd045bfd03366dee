#!/usr/bin/env python3
"""Digests of the kernel-level dispatch, for comparing two builds of the library call for call.

Runs a fixed table of attention and GEMM calls in this (fresh) process, in a fixed order, on seeded operands, and prints one JSON line:
the sha256 of every output, by call.  The table reaches every host-side branch that picks a kernel or a launch plan:

  bf16 attention, in both libraries (bfloat16, float16); (nseq, H, sq, sk per chunk, chunks):
    a short stream in the 4-wave geometry (1, 2, 300, 300, 1); the resident key stream (16, 8, 1030, 144, 1) and, with no tail tile,
    (16, 8, 1030, 128, 1); three chunks on the 4x64 kernel (1, 2, 520, 1100, 3) and on the balanced kernel (code 78: the chunk advance of
    its two DMA cursors); the split tail (1, 2, 2320, 4200, 1) and (1, 1, 2432, 4097, 1) with exactly 128 tail rows; a short last
    block that is not split (1, 2, 2320, 300, 1); the two-pass sequence rows = 1 / state_mode 1 -> state_mode 2 -> rows = 2 at
    (2, 2, 2320, 1100, 4); the forced kernels 28, 58, 60, 68, 78, 90, 98 at (1, 2, 520, 1100, 1)
  fp8 attention: forms 0, 100, 200, 400 at (1, 2, 2320, 2320, 1), (2, 1, 300, 4111, 2) and (1, 1, 256, 577, 1); a stream under 8 tiles
    (1, 2, 300, 257, 1; not form 100, which the entry refuses there); a key stream whose last tile is full, so that no key is masked,
    (1, 1, 256, 576, 1) and under 8 tiles (1, 2, 300, 256, 1); the two-pass sequence; the split tail
  the partials scratch of either family: a split tail at nseq * H = 1 early, one at nseq * H = 4 later (the buffer grows: this process
    is fresh), then the first call again - asserted to give the first call's digest
  GEMM: every case of tests/_gemm_exact.CASES through the call tests/test_gemm_exact_gpu.py makes, in both libraries; ops.gemm_head_post
    at a shape that fuses and has remainder rows (M = 4112, N = 3072, K = 64) and at one that falls back to the two calls (M = 512)

--launches DIR reads the kernel trace of a run of this script under `rocprofv3 --kernel-trace -d DIR -- python tools/dispatch_digest.py`
instead and prints the length and the sha256 of the ordered list of (kernel name, grid, workgroup, LDS bytes), the runtime's copy
kernels left out.
"""
import argparse
import glob
import hashlib
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORCED = (28, 58, 60, 68, 78, 90, 98)
FP8_FORMS = (0, 100, 200, 400)


def launches(directory):
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True))
    assert len(dbs) == 1, dbs
    c = sqlite3.connect(dbs[0])
    have = [r[1] for r in c.execute("pragma table_info(kernels)")]
    cols = ["name"] + [f"{w}_{ax}" for w in ("grid", "workgroup") for ax in "xyz"] + ["lds_size"]
    assert all(x in have for x in cols + ["start"]), have
    # the runtime's own blit kernels are not launches of the program: whether a host-to-device copy runs as one is the runtime's choice
    rows = [list(r) for r in c.execute(f"select {', '.join(cols)} from kernels order by start") if not r[0].startswith("__amd_rocclr_")]
    text = json.dumps(rows).encode()
    return {"launches": len(rows), "sha256": hashlib.sha256(text).hexdigest(),
            "library_launches": sum("attn" in r[0] or "gemm" in r[0] or "quant" in r[0] or "head_post" in r[0] for r in rows)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", metavar="DIR")
    a = ap.parse_args()
    if a.launches:
        print(json.dumps(launches(a.launches)))
        return

    import torch
    from actionmesh_amd import ops
    import _gemm_exact as X
    import test_gemm_exact_gpu as G

    assert torch.cuda.is_available(), "dispatch_digest.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {}

    def sha(*ts):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in ts:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        return h.hexdigest()

    def record(key, *ts):
        assert key not in res, key
        res[key] = sha(*ts)
        return res[key]

    def operands(nseq, H, sq, skc, P, dtype):
        """Seeded padded operands of ops.attention: keys in P chunks of skc, pad rows zero."""
        g = torch.Generator().manual_seed(1000 * sq + skc + P)
        sq_pad, sk_pad = ops.round_up(sq, 256), ops.round_up(skc, 64)
        Q = torch.zeros((nseq, H, sq_pad, 128), dtype=dtype)
        Q[:, :, :sq] = (torch.randn((nseq, H, sq, 128), generator=g) * 1.3).to(dtype)
        K = torch.zeros((P, nseq, H, sk_pad, 128), dtype=dtype)
        K[:, :, :, :skc] = torch.randn((P, nseq, H, skc, 128), generator=g).to(dtype)
        V = torch.zeros((P, nseq, H, sk_pad, 128), dtype=dtype)
        V[:, :, :, :skc] = torch.randn((P, nseq, H, skc, 128), generator=g).to(dtype)
        Vt = V[:, :, :, ops.perm16_index(sk_pad, "cpu")].transpose(-1, -2).contiguous()
        return Q.to(dev), K.to(dev), Vt.to(dev)

    def two_pass(attend, key, shape, dtype, **kw):
        nseq, H, sq, skc, P = shape
        Q, K, Vt = operands(*shape, dtype)
        if attend is ops.attention_fp8:          # the passes share one quantisation, as the model's do
            record(key + " one pass", attend(Q, K, Vt, sq, skc, nchunks=P, **kw))
            kw["quantized"] = ops.attention_fp8.last_quantized
        state = torch.zeros((nseq * H, Q.shape[2], ops.STATE_LD), device=dev)
        out = torch.full((nseq * sq, H * 128), 768.0, dtype=dtype, device=dev)
        attend(Q, K, Vt, sq, skc, out=out, nchunks=1, rows=1, state_mode=1, state=state, chunk_first=1, chunk_total=P, **kw)
        record(key + " state", state)
        attend(Q, K, Vt, sq, skc, out=out, nchunks=P - 1, rows=1, state_mode=2, state=state, chunk_first=2 % P, chunk_total=P, **kw)
        attend(Q, K, Vt, sq, skc, out=out, nchunks=P, rows=2, **kw)
        record(key, out)

    # ---- bf16 attention, both libraries -----------------------------------------------------------------------------------------
    for name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        def attn(key, shape, **kw):
            nseq, H, sq, skc, P = shape
            Q, K, Vt = operands(*shape, dtype)
            return record(f"attention {name} {key} {shape}", ops.attention(Q, K, Vt, sq, skc, nchunks=P, **kw))

        first = attn("split tail of 128 rows, nseq*H = 1", (1, 1, 2432, 4097, 1))
        for defer in (0, 8):
            attn(f"short stream defer={defer}", (1, 2, 300, 300, 1), defer_log2=defer)
            attn(f"resident defer={defer}", (16, 8, 1030, 144, 1), defer_log2=defer)
            attn(f"resident, no tail tile defer={defer}", (16, 8, 1030, 128, 1), defer_log2=defer)
            attn(f"three chunks defer={defer}", (1, 2, 520, 1100, 3), defer_log2=defer)
            attn(f"split tail defer={defer}", (1, 2, 2320, 4200, 1), defer_log2=defer)
            attn(f"short last block, not split defer={defer}", (1, 2, 2320, 300, 1), defer_log2=defer)
            two_pass(ops.attention, f"attention {name} two-pass defer={defer}", (2, 2, 2320, 1100, 4), dtype, defer_log2=defer)
        for code in FORCED:
            attn(f"code {code}", (1, 2, 520, 1100, 1), defer_log2=code)
        attn("code 78, three chunks", (1, 2, 520, 1100, 3), defer_log2=78)
        attn("split tail, nseq*H = 4", (2, 2, 2320, 4200, 1))
        again = sha(ops.attention(*operands(1, 1, 2432, 4097, 1, dtype), 2432, 4097))
        assert again == first, f"{name}: the split tail changed its output after the partials scratch grew"
        res[f"attention {name} split tail of 128 rows again"] = again

    # ---- fp8 attention ----------------------------------------------------------------------------------------------------------------
    def attn8(key, shape, **kw):
        nseq, H, sq, skc, P = shape
        Q, K, Vt = operands(*shape, torch.bfloat16)
        return record(f"attention fp8 {key} {shape}", ops.attention_fp8(Q, K, Vt, sq, skc, nchunks=P, **kw))

    first = attn8("split tail of 128 rows, nseq*H = 1", (1, 1, 2432, 4097, 1))
    for form in FP8_FORMS:
        for shape in ((1, 2, 2320, 2320, 1), (2, 1, 300, 4111, 2), (1, 1, 256, 577, 1)):
            attn8(f"form {form}", shape, ablate=form)
        attn8(f"full last tile form {form}", (1, 1, 256, 576, 1), ablate=form)      # no key past the chunk's end: the mask branch is not taken
        if form != 100:      # the 4 x 64 form has no kernel for a stream under 8 tiles: the entry refuses the code there
            attn8(f"under 8 tiles form {form}", (1, 2, 300, 257, 1), ablate=form)
            attn8(f"under 8 tiles, full last tile form {form}", (1, 2, 300, 256, 1), ablate=form)
        two_pass(ops.attention_fp8, f"attention fp8 two-pass form {form}", (2, 2, 2320, 1100, 4), torch.bfloat16, ablate=form)
    attn8("split tail", (1, 2, 2320, 4200, 1))
    attn8("split tail, nseq*H = 4", (2, 2, 2320, 4200, 1))
    again = sha(ops.attention_fp8(*operands(1, 1, 2432, 4097, 1, torch.bfloat16), 2432, 4097))
    assert again == first, "fp8: the split tail changed its output after the partials scratch grew"
    res["attention fp8 split tail of 128 rows again"] = again

    # ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
    for name in X.DTYPES:
        for case in X.CASES:
            c, _, _ = X.operands(case, name)
            record(f"gemm {name} {X.case_id(case)}", G._run(c, dev))
    X._a_w.cache_clear()
    for name, dtype in X.DTYPES.items():
        for M, frames in ((4112, 16), (512, 4)):
            g = torch.Generator().manual_seed(M)
            a = torch.randn((M, 64), generator=g).to(dtype).to(dev)
            w = (torch.randn((3072, 64), generator=g) * 0.125).to(dtype).to(dev)
            wq, wk = ((torch.randn((128,), generator=g) * 0.2 + 1.0).to(dev) for _ in range(2))
            ang = torch.arange(frames)[:, None].float() * (10000.0 ** (-torch.arange(64).float() * 2 / 128))[None]
            rope = (torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev))
            fill = torch.full((1,), -3.0, dtype=dtype, device=dev)
            outs = [fill.expand(s).contiguous() for s in ((1, 8, ops.round_up(M, 256), 128), (1, 8, ops.round_up(M, 64), 128),
                                                          (1, 8, 128, ops.round_up(M, 64)))]
            x = fill.expand(M, 3072).contiguous()
            ops.gemm_head_post(a, w, 8, (0, 1, 2), M, M // frames, w_q=wq, w_k=wk, rope=rope, out_q=outs[0], out_k=outs[1], out_vt=outs[2],
                               x=x)
            record(f"gemm_head_post {name} M={M}", *outs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
