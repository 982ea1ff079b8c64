"""Which model-fit kernel abc_pls_model_dev runs, and which of its internal branches: a copy of launch_pls_model() in
abcsmc_amd/csrc/pls.hip, so that a test can state the instantiation and branches it means to reach and check that it does.
tests/test_pls_dispatch.py holds this copy against the PLS_LAUNCH / PLS_LAUNCH_NB / FIT16_LAUNCH sites of pls.hip;
tests/test_gpu_pls_model.py asserts through it that its cases reach every instantiation and branch.

Instantiations (the `kernel` of fit_plan):
    ("fit", NW, GMEM, NB)   k_pls_fit<NW, GMEM, NB>: one work-group of NW waves; GMEM: the work arrays in global memory;
                            NB 1 / 2: the register-resident eigen-squaring on 16 NB x 16 NB blocks, 0: 4 x 4 blocks or, beyond 64
                            responses, the memory-resident one
    ("fit16", NW, NB)       k_pls_fit16<NW, NB>: the latency-tuned fit, 2..32 responses
"""

LDS_LIMIT = 160 * 1024          # bytes of LDS a work-group may take (launch_pls_model)


def nb_of(P):
    """the NB template argument PLS_LAUNCH_NB picks"""
    return 1 if P <= 16 else 2 if P <= 32 else 0


def lds_fit_doubles(M, P, A):
    """lds_d of launch_pls_model: k_pls_fit's work arrays"""
    xx_in_lds = M <= 64
    return (M * P + 2 * P * P + P + 4 * M + 2 * M * A + (M * M if xx_in_lds else 0) + 8 + (8 + A + 4 * M)
            + (P * P + P if P > 64 else 0) + (8 * 256 if P <= 16 else 0))


def lds_fit16_doubles(M, P, A):
    """lds16_d of launch_pls_model: k_pls_fit16's LDS"""
    nb16 = 1 if P <= 16 else 2
    xx_in_lds = M <= 64
    return ((M + 3) * P + 16 * nb16 + 3 * M + 4 + 4 * M + 128 * nb16 + A + 2 * M * A + (8 if M > 64 else 4) * 256 * nb16 * nb16
            + (M * M if xx_in_lds else 0) + A * A + 3 * P * A + (2048 if nb16 == 2 else 0))


def fit_plan(M, P, A):
    """-> dict: kernel (see the module docstring), fold_z (k_pls_fit16 runs k_zstats' work as its prologue), and the internal
    branches the fit takes:
        eig     None (P == 1: w = XY), "square1" / "square2" / "square4" (eig_square<NB> or k_pls_fit16's squaring on NB x NB
                blocks), "generic" (eig_generic: NB == 0 and more than 64 responses)
        xx      where X'X (training) is read from: "lds" (M <= 64), "reg" (quarter rows in registers, eight waves, M <= 128),
                "global"
        press   "gemm" (pls_gemm on the matrix pipe: A M >= 1024) or "entry" (one thread per entry)
        q8      k_pls_fit only: q = XY'r / tt by eight threads per response (NW > 1, M > 64, 4 M >= 8 P)
    """
    xx_in_lds = M <= 64
    gbase = lds_fit_doubles(M, P, A) * 8 > LDS_LIMIT
    nb16 = 1 if P <= 16 else 2
    fit16 = 2 <= P <= 32 and M > 16 and lds_fit16_doubles(M, P, A) * 8 <= LDS_LIMIT
    fold_z = fit16 and M * (M + P) <= 4096
    press = "gemm" if A * M >= 1024 else "entry"
    if fit16:
        NW = 8 if M > 64 else 4
        kernel = ("fit16", NW, nb16)
        xx = "lds" if xx_in_lds else "reg" if (NW == 8 and nb16 == 1 and M <= 128) else "global"
        return {"kernel": kernel, "fold_z": fold_z, "eig": "square%d" % nb16, "xx": xx, "press": press, "q8": False}
    if gbase:
        kernel = ("fit", 8, True, 1 if P <= 16 else 0)
    elif M > 64:
        kernel = ("fit", 8, False, nb_of(P))
    elif M > 16:
        kernel = ("fit", 4, False, nb_of(P))
    else:
        kernel = ("fit", 1, False, nb_of(P))
    _, NW, GMEM, NB = kernel
    if P == 1:
        eig = None
    elif NB == 0 and P > 64:
        eig = "generic"
    else:
        eig = "square%d" % (NB or 4)
    xx = "lds" if xx_in_lds else "reg" if (NW == 8 and not GMEM and M <= 128) else "global"
    q8 = NW > 1 and M > 64 and 4 * M >= 8 * P
    return {"kernel": kernel, "fold_z": False, "eig": eig, "xx": xx, "press": press, "q8": q8}


def reachable(max_m=260, max_p=140):
    """every instantiation launch_pls_model can reach over M, P up to the given sizes (A = 1, 8 and M)"""
    out = set()
    for M in range(1, max_m + 1):
        for P in range(1, max_p + 1):
            for A in sorted({1, min(8, M), M}):
                out.add(fit_plan(M, P, A)["kernel"])
    return out
