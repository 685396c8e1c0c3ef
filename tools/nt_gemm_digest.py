"""SHA-256 of every output of the 16-bit NT GEMM family on seeded operands: one line per (problem, epilogue, tensor).

Two libraries compute the same thing exactly when their lines are equal:

    python tools/nt_gemm_digest.py > head.txt
    SPE_HIP_LIB=/path/to/other/libspe_hip.so python tools/nt_gemm_digest.py > other.txt
    python tools/nt_gemm_digest.py --compare other.txt head.txt

Problems: GPU_CASES and STEP_SHAPES of tests/nt_gemm_cases.py (every kernel instance; the NT products of a cfg2 step).  Epilogues: the
combinations spe_amd/kernels.py and spe_amd/ops.py issue - plain: no bias (input gradients) / bias / bias + activation + pre-activation
copy / fp16 operands with fp16 output; extended: LayerScale residual, fc1 + GELU with the second 16-bit copy, dh (activation derivative,
bf16 result, column sums), each also with dropout (and the per-sample scale) inside the epilogue, and the transposed copy where the
problem asks for one.  --compare lists unequal lines; column sums (`colsum`) are reported separately, since their last bits may
depend on the row-tile height when two libraries choose different tiles for a problem."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(a, b):
    rows = [dict(l.split(" = ") for l in open(f) if l.startswith("DIGEST ")) for f in (a, b)]
    keys = sorted(set(rows[0]) | set(rows[1]))
    bad = [k for k in keys if rows[0].get(k) != rows[1].get(k)]
    cs = [k for k in bad if k.endswith(" colsum")]
    print(f"{len(keys)} digests, {len(keys) - len(bad)} equal, {len(bad) - len(cs)} unequal outputs, {len(cs)} unequal column sums")
    for k in bad:
        print("UNEQUAL", k)
    return 1 if len(bad) > len(cs) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    import ctypes

    import torch
    import nt_gemm_cases as C
    from spe_amd import lib
    if not hasattr(ctypes.CDLL(lib.LIBPATH), "spe_gemm_bf16nt_plan"):      # a library from before the plan entry: the GEMM entries are all this needs
        lib.PROTOS.pop("spe_gemm_bf16nt_plan")
    from spe_amd import kernels as K
    dev = torch.device("cuda:0")
    have_plan = "spe_gemm_bf16nt_plan" in lib.PROTOS

    def emit(tag, combo, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            if t is not None:
                print(f"DIGEST {tag} {combo} {name} = {hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()}", flush=True)

    seen = []
    for case in C.GPU_CASES + C.STEP_SHAPES:
        if case in seen:
            continue
        seen.append(case)
        M, N, Kd = case["M"], case["N"], case["K"]
        split, ex, f16, want_T = (bool(case.get(k)) for k in ("split", "ex", "op_f16", "out16T"))
        tag = "x".join(map(str, (M, N, Kd))) + "".join("-" + k for k in ("split", "ex", "op_f16", "out16T") if case.get(k))
        if have_plan:
            print(f"PLAN {tag} {C.kernel_name(K.gemm16_plan(M, N, Kd, **{k: v for k, v in case.items() if k not in 'MNK'}))}")
        g = torch.Generator().manual_seed(M * 7 + N * 3 + Kd)
        x = torch.randn(M, Kd, generator=g).to(dev); W = (torch.randn(N, Kd, generator=g) / Kd ** 0.5).to(dev); b = torch.randn(N, generator=g).to(dev)
        res = torch.randn(M, N, generator=g).to(dev); gam = torch.rand(N, generator=g).to(dev); aux = torch.randn(M, N, generator=g).to(dev)
        ss = (torch.rand(4, generator=g) + 0.5).to(dev); rps = (M + 3) // 4
        new = lambda dt=torch.float32: torch.zeros((M, N), device=dev, dtype=dt)
        if f16:
            A, B, lo = K.cvt_f16(x), K.cvt_f16(W), {}
        else:
            A, B = x.to(torch.bfloat16), W.to(torch.bfloat16)
            lo = dict(Alo=(x - A.float()).to(torch.bfloat16), Blo=(W - B.float()).to(torch.bfloat16)) if split else {}
        if not ex and f16:
            y = new(torch.float16)
            K.gemm16(A, B, y, M, N, Kd, Kd, Kd, N, bias=b, act=0x300)
            emit(tag, "f16out", C=y)
        elif not ex:
            c = new(); K.gemm16(A, B, c, M, N, Kd, Kd, Kd, N, **lo); emit(tag, "nobias", C=c)
            c = new(); K.gemm16(A, B, c, M, N, Kd, Kd, Kd, N, bias=b, **lo); emit(tag, "bias", C=c)
            for act in (1, 2):
                c, c2 = new(), new(); K.gemm16(A, B, c, M, N, Kd, Kd, Kd, N, bias=b, C2=c2, act=act, **lo); emit(tag, f"act{act}", C=c, C2=c2)
        else:
            f = dict(op_f16=True) if f16 else {}
            for nm, dr in (("", {}), ("+drop", dict(drop=(0.1, 1234, 64), sscale=ss, rps=rps))):
                out, y, o16 = new(), new(), new(torch.bfloat16)
                o16T = torch.zeros((N, case["ld16t"]), device=dev, dtype=torch.bfloat16) if want_T else None
                K.gemm16_ex(A, B, M, N, Kd, Kd, Kd, bias=b, C=out, C2=y, out16=o16, out16T=o16T, res=res, rgamma=gam, **lo, **f, **dr)
                emit(tag, "residual" + nm, C=out, C2=y, out16=o16, out16T=o16T)
            for nm, dr in (("", {}), ("+drop", dict(drop=(0.1, 1234, 64)))):
                if split or f16:
                    pre, h, h2 = new(), new(torch.bfloat16), new(torch.float16 if f16 else torch.bfloat16)
                    K.gemm16_ex(A, B, M, N, Kd, Kd, Kd, bias=b, C2=pre, out16=h, act=2, out16lo=h2, **lo, **f, **dr)
                    emit(tag, "fc1" + nm, C2=pre, out16=h, out16lo=h2)
                else:
                    d16, cs = new(torch.bfloat16), torch.zeros(N, device=dev)
                    K.gemm16_ex(A, B, M, N, Kd, Kd, Kd, out16=d16, colsum=cs, aux=aux, act=2, **dr)
                    emit(tag, "dh" + nm, out16=d16, colsum=cs)


if __name__ == "__main__":
    main()
