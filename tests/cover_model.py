"""An independent model of the coverage base counters (csrc/cover.h), in the
oracle's canonical-tuple space: numpy only, no product code.

cover(tuples, nc, np_, ns) sums, over the given states, the per-state vector
DESIGN.md §4.9 defines.  Every state is taken as one that the BFS expands:
TLC evaluates Next once on it, and each counter is what one sub-expression of
KubeAPI.tla adds to its evaluation count there.

Tuple layout (oracle/kubeapi_oracle.c to_tuple): word 0 apiState (a mask over
the object universe U, u = id << (R+1) | spec << R | vv, R = nc + np), then 19
words per process.  Sets are enumerated in ascending u, which is TLC's order
for Model_1's at most two stored objects (the Secret before the PVC).
"""
from __future__ import annotations

import numpy as np

ACTIONS = [
    "DoRequest", "DoReply", "DoListRequest", "DoListReply", "CStart", "C1", "C10", "C11",
    "c12", "C13", "C2", "C3", "C8", "C6", "C7", "C4", "C5", "PVCStart", "PVCListedPVCs",
    "PVCHavePVCs", "PVCDone", "APIStart",
]
BRANCHES = [
    "CSTART_THEN", "CSTART_ELSE", "C1_START", "C1_C10", "C11_START", "C11_c12", "C13_START",
    "C13_C2", "C3_START", "C3_C8", "C8_C4", "C8_C6", "C7_START", "C7_C4", "PVCL_START",
    "PVCL_HAVE", "API_CREATE", "API_FORCE", "API_FORCE_REPLACE", "API_FORCE_CREATE", "API_GET",
    "API_GET_NOTFOUND", "API_DELETE", "API_UPDATE", "API_UPDATE_OK", "API_UPDATE_ERR",
    "API_LIST", "API_ASSERT",
]
COV = ["cov_api", "cov_req", "cov_lreq", "cov_objs", "cov_api2"]
EXTRA = [
    "en_DoReply", "en_DoListReply", "en_APIStart", "states",
    "c13_ok", "c13_pvc", "c13_spec", "c7_ok", "c4_iter",
    "pvcl_ok", "pvcl_objs", "pvcl_objs_pvc", "pvcl_objs_spec",
    "create_exists", "force_iter", "force_setsz", "force_same",
    "get_iter", "get_iter_found", "get_setsz", "get_same",
    "del_setsz", "del_same", "upd_iter", "upd_nmatch", "upd_setsz", "upd_same",
    "list_setsz", "list_match",
]
NAMES = ["B_" + b for b in BRANCHES] + COV + ["pairs_" + a for a in ACTIONS] + EXTRA

# labels (oracle/kubeapi_oracle.h KO_*), verbs, responses, kinds
(PC_CStart, PC_C1, PC_C10, PC_C11, PC_c12, PC_C13, PC_C2, PC_C3, PC_C8, PC_C6, PC_C7, PC_C4, PC_C5,
 PC_PVCStart, PC_PVCListedPVCs, PC_PVCHavePVCs, PC_PVCDone, PC_APIStart,
 PC_DoRequest, PC_DoReply, PC_DoListRequest, PC_DoListReply) = range(1, 23)
PC_OF_ACTION = [PC_DoRequest, PC_DoReply, PC_DoListRequest, PC_DoListReply, PC_CStart, PC_C1, PC_C10,
                PC_C11, PC_c12, PC_C13, PC_C2, PC_C3, PC_C8, PC_C6, PC_C7, PC_C4, PC_C5, PC_PVCStart,
                PC_PVCListedPVCs, PC_PVCHavePVCs, PC_PVCDone, PC_APIStart]
OP_Create, OP_Get, OP_Update, OP_Delete, OP_Force = 1, 2, 3, 4, 5
ST_Pending, ST_Ok, ST_Error = 1, 2, 3
K_Secret, K_PVC = 1, 2
# per-process tuple fields
F_PC, F_SR, F_RQP, F_RQOP, F_RQST, F_RQOBJ, F_LRP, F_LRK, F_LRST, F_LROBJS = 0, 4, 11, 12, 13, 14, 15, 16, 17, 18
PER_PROC = 19


def popc(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8).reshape(-1, 8)
    return np.unpackbits(b, axis=1).sum(axis=1).astype(np.int64)


def upto_first(m: np.ndarray) -> np.ndarray:
    """Mask of the bits up to and including the lowest set bit of m (all ones if m == 0)."""
    m = m.astype(np.uint64)
    low = m & (~m + np.uint64(1))
    return np.where(m != 0, (low << np.uint64(1)) - np.uint64(1), np.uint64(0xFFFFFFFFFFFFFFFF)).astype(np.uint64)


def cover(tuples: np.ndarray, nc: int = 1, np_: int = 1, ns: int = 1, variant: int = 0) -> dict:
    t = np.ascontiguousarray(tuples, dtype=np.uint64)
    P, R = nc + np_ + ns, nc + np_
    assert t.ndim == 2 and t.shape[1] == 1 + PER_PROC * P
    n = t.shape[0]
    usz = 1 << (R + 1)
    idm = [np.uint64((1 << usz) - 1), np.uint64(((1 << usz) - 1) << usz)]
    spec_m = np.uint64(sum(1 << u for u in range(2 * usz) if (u >> R) & 1))
    api = t[:, 0] & (idm[0] | idm[1])
    napi = popc(api)
    c = {k: 0 for k in NAMES}

    def fld(p, f):
        return t[:, 1 + PER_PROC * p + f]

    def tot(mask, w=None):
        return int(mask.sum()) if w is None else int((w * mask).sum())

    c["states"] = n
    c["cov_api"] = int(napi.sum())
    c["cov_api2"] = int((napi * napi).sum())
    pend_rq = np.zeros(n, dtype=bool)
    pend_lr = np.zeros(n, dtype=bool)
    for p in range(P):
        pc = fld(p, F_PC).astype(np.int64)
        rqp, rqst, rqop = fld(p, F_RQP) != 0, fld(p, F_RQST).astype(np.int64), fld(p, F_RQOP).astype(np.int64)
        lrp, lrst, lrk = fld(p, F_LRP) != 0, fld(p, F_LRST).astype(np.int64), fld(p, F_LRK).astype(np.int64)
        rqobj = fld(p, F_RQOBJ).astype(np.int64)
        objs = fld(p, F_LROBJS)
        nobjs = popc(objs)
        c["cov_req"] += tot(rqp)
        c["cov_lreq"] += tot(lrp)
        c["cov_objs"] += tot(lrp, nobjs)
        for a in range(4):
            c["pairs_" + ACTIONS[a]] += tot(pc == PC_OF_ACTION[a])
        c["en_DoReply"] += tot((pc == PC_DoReply) & (rqst != ST_Pending))
        c["en_DoListReply"] += tot((pc == PC_DoListReply) & (lrst != ST_Pending))
        if p < nc:
            for a in range(4, 17):
                c["pairs_" + ACTIONS[a]] += tot(pc == PC_OF_ACTION[a])
            at = pc == PC_CStart
            sr = fld(p, F_SR) != 0
            c["B_CSTART_THEN"] += tot(at) + tot(at & sr)
            c["B_CSTART_ELSE"] += tot(at & ~sr)
            ok = rqst == ST_Ok
            at = pc == PC_C1
            back = ~ok if variant != 3 else np.zeros(n, dtype=bool)
            c["B_C1_START"] += tot(at & back)
            c["B_C1_C10"] += tot(at & ~back)
            at = pc == PC_C11
            c["B_C11_START"] += tot(at & ~ok)
            c["B_C11_c12"] += tot(at & ok)
            at = pc == PC_C13
            ispvc = ((rqobj >> 1) & 1) == 1
            spec = ((rqobj >> 3) & 1) == 1
            unbound = ispvc & ~spec
            c["c13_ok"] += tot(at & ok)
            c["c13_pvc"] += tot(at & ok & ispvc)
            c["c13_spec"] += tot(at & ok & ispvc & spec)
            c["B_C13_START"] += tot(at & (~ok | unbound))
            c["B_C13_C2"] += tot(at & ok & ~unbound)
            lok = lrst == ST_Ok
            at = pc == PC_C3
            c["B_C3_START"] += tot(at & ~lok)
            c["B_C3_C8"] += tot(at & lok)
            at = pc == PC_C8
            c["B_C8_C4"] += tot(at & (objs == 0))
            c["B_C8_C6"] += tot(at & (objs != 0))
            at = pc == PC_C7
            c["c7_ok"] += tot(at & ok)
            c["B_C7_START"] += tot(at & (~ok | (nobjs > 1)))
            c["B_C7_C4"] += tot(at & ok & (nobjs <= 1))
            at = pc == PC_C4
            c["c4_iter"] += tot(at, popc(api & upto_first(api & idm[0])))
        elif p < R:
            for a in range(17, 21):
                c["pairs_" + ACTIONS[a]] += tot(pc == PC_OF_ACTION[a])
            at = pc == PC_PVCListedPVCs
            lok = lrst == ST_Ok
            unb = objs & idm[1] & ~spec_m
            c["pvcl_ok"] += tot(at & lok)
            c["pvcl_objs"] += tot(at & lok, nobjs)
            c["pvcl_objs_pvc"] += tot(at & lok, popc(objs & idm[1]))
            c["pvcl_objs_spec"] += tot(at & lok, popc(objs & idm[1] & spec_m))
            c["B_PVCL_START"] += tot(at & (~lok | (unb == 0)))
            c["B_PVCL_HAVE"] += tot(at & lok & (unb != 0))
        else:
            c["pairs_APIStart"] += n
        # APIStart's view of process p's pending request / list request, once per server
        pr = rqp & (rqst == ST_Pending)
        pend_rq |= pr
        rid = (rqobj >> 1) & 1
        same = api & np.where(rid == 1, idm[1], idm[0])
        nsame = popc(same)
        has = same != 0
        m = pr & (rqop == OP_Create)
        c["B_API_CREATE"] += ns * tot(m)
        c["create_exists"] += ns * tot(m & has)
        m = pr & (rqop == OP_Force)
        c["B_API_FORCE"] += ns * tot(m)
        c["B_API_FORCE_REPLACE"] += ns * tot(m & has)
        c["B_API_FORCE_CREATE"] += ns * tot(m & ~has)
        c["force_iter"] += ns * tot(m, popc(api & upto_first(same)))
        c["force_setsz"] += ns * tot(m & has, napi)
        c["force_same"] += ns * tot(m & has, nsame)
        m = pr & (rqop == OP_Get)
        c["B_API_GET"] += ns * tot(m)
        c["B_API_GET_NOTFOUND"] += ns * tot(m & ~has)
        it = popc(api & upto_first(same))
        c["get_iter"] += ns * tot(m, it)
        c["get_iter_found"] += ns * tot(m & has, it)
        c["get_setsz"] += ns * tot(m & has, napi)
        c["get_same"] += ns * tot(m & has, nsame)
        m = pr & (rqop == OP_Delete)
        c["B_API_DELETE"] += ns * tot(m)
        c["del_setsz"] += ns * tot(m, napi)
        c["del_same"] += ns * tot(m, nsame)
        m = pr & (rqop == OP_Update)
        c["B_API_UPDATE"] += ns * tot(m)
        if p < R:
            readm = np.uint64(sum(1 << u for u in range(2 * usz) if (u >> p) & 1))
        else:
            readm = np.uint64(0)
        hit = same & readm
        ok = (hit != 0) | (has if variant == 1 else np.zeros(n, dtype=bool))
        c["B_API_UPDATE_OK"] += ns * tot(m & ok)
        c["B_API_UPDATE_ERR"] += ns * tot(m & ~ok)
        up = upto_first(hit)
        c["upd_iter"] += ns * tot(m, popc(api & up))
        c["upd_nmatch"] += ns * tot(m, popc(same & up))
        c["upd_setsz"] += ns * tot(m & ok, napi)
        c["upd_same"] += ns * tot(m & ok, nsame)
        m = pr & ((rqop < OP_Create) | (rqop > OP_Force))
        c["B_API_ASSERT"] += ns * tot(m)
        pl = lrp & (lrst == ST_Pending)
        pend_lr |= pl
        km = np.where(lrk == K_Secret, idm[0], np.where(lrk == K_PVC, idm[1], np.uint64(0))).astype(np.uint64)
        c["B_API_LIST"] += ns * tot(pl)
        c["list_setsz"] += ns * tot(pl, napi)
        c["list_match"] += ns * tot(pl, popc(api & km))
    c["en_APIStart"] = ns * tot(pend_rq | pend_lr)
    return c


def add(a: dict, b: dict) -> dict:
    return {k: a.get(k, 0) + b[k] for k in b}
