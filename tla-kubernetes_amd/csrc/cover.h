// cover.h — expression-level coverage (TLC's -coverage) of KubeAPI.tla as a
// fixed vector of base counters per expanded state.
//
// TLC evaluates Next once on every state it dequeues, and every count of its
// coverage block (MC.out msg 2221/2775) is the sum over those states of how
// often one sub-expression was evaluated there.  cover_visit<M> is that
// per-state contribution for the KC_COVER_N base counters below; every line
// TLC prints is a fixed integer combination of their sums, of act_gen[22], of
// the Init count and of the sizes of the self sets (kubecheck/tlc.py,
// COVERAGE_LINES).  Kernels and host run the same code (KC_HD), as
// live_stay<M> does.
//
// Sets are enumerated in ascending u (kubeapi_spec.h), which is TLC's order
// of apiState's elements in the reference run: the Secret before the PVC
// (MC.out:717-738: every Get of the PVC evaluates IsVersionOf twice).  An
// \E or CHOOSE over apiState stops at its first match; a set comprehension
// visits every element.
#pragma once
#include "kubeapi_spec.h"

namespace kc {

enum CoverIdx : int {
  // IF / CASE branch counts: the oracle's KO_B_* (oracle/kubeapi_oracle.h), same order and meaning
  CV_B_CSTART_THEN = 0, CV_B_CSTART_ELSE, CV_B_C1_START, CV_B_C1_C10, CV_B_C11_START, CV_B_C11_c12,
  CV_B_C13_START, CV_B_C13_C2, CV_B_C3_START, CV_B_C3_C8, CV_B_C8_C4, CV_B_C8_C6, CV_B_C7_START,
  CV_B_C7_C4, CV_B_PVCL_START, CV_B_PVCL_HAVE, CV_B_API_CREATE, CV_B_API_FORCE, CV_B_API_FORCE_REPLACE,
  CV_B_API_FORCE_CREATE, CV_B_API_GET, CV_B_API_GET_NOTFOUND, CV_B_API_DELETE, CV_B_API_UPDATE,
  CV_B_API_UPDATE_OK, CV_B_API_UPDATE_ERR, CV_B_API_LIST, CV_B_API_ASSERT,
  // the invariants' quantifier bodies: the oracle's cov_* sums
  CV_COV_API, CV_COV_REQ, CV_COV_LREQ, CV_COV_OBJS, CV_COV_API2,
  // (state, self) pairs at each action's label, in action order
  CV_PAIRS,
  // pairs whose action is enabled, where that is less than the pairs at the label
  CV_EN_DOREPLY = CV_PAIRS + A_COUNT, CV_EN_DOLISTREPLY, CV_EN_APISTART,
  CV_STATES,                              // states expanded
  // C13 (:590): requests[self].status = "Ok"; ... and the object is a PVC; ... with a spec
  CV_C13_OK, CV_C13_PVC, CV_C13_SPEC,
  CV_C7_OK,                               // C7 (:632): status = "Ok"
  CV_C4_ITER,                             // C4 (:639, :410): bodies of \E o \in apiState
  // PVCListedPVCs (:667): status = "Ok"; sum of |objs|; of its PVCs; of its PVCs with a spec
  CV_PVCL_OK, CV_PVCL_OBJS, CV_PVCL_OBJS_PVC, CV_PVCL_OBJS_SPEC,
  CV_CREATE_EXISTS,                       // APIStart Create (:701): the object exists
  // Force (:707-713): \E bodies; sum |apiState| and |versions of the object| where it exists
  CV_FORCE_ITER, CV_FORCE_SETSZ, CV_FORCE_SAME,
  // Get (:717-726): \E bodies; CHOOSE bodies (found only); sum |apiState|, |versions| when found
  CV_GET_ITER, CV_GET_ITER_FOUND, CV_GET_SETSZ, CV_GET_SAME,
  CV_DEL_SETSZ, CV_DEL_SAME,              // Delete (:730)
  // Update (:733-736): \E bodies; versions met by them; sum |apiState|, |versions| when applied
  CV_UPD_ITER, CV_UPD_NMATCH, CV_UPD_SETSZ, CV_UPD_SAME,
  CV_LIST_SETSZ, CV_LIST_MATCH,           // list requests (:746-752): sum |apiState|, |objects of the kind|
  KC_COVER_N
};

inline const char* cover_name(int i) {
  static const char* const kNames[KC_COVER_N] = {
      "B_CSTART_THEN", "B_CSTART_ELSE", "B_C1_START", "B_C1_C10", "B_C11_START", "B_C11_c12", "B_C13_START",
      "B_C13_C2", "B_C3_START", "B_C3_C8", "B_C8_C4", "B_C8_C6", "B_C7_START", "B_C7_C4", "B_PVCL_START",
      "B_PVCL_HAVE", "B_API_CREATE", "B_API_FORCE", "B_API_FORCE_REPLACE", "B_API_FORCE_CREATE", "B_API_GET",
      "B_API_GET_NOTFOUND", "B_API_DELETE", "B_API_UPDATE", "B_API_UPDATE_OK", "B_API_UPDATE_ERR", "B_API_LIST",
      "B_API_ASSERT",
      "cov_api", "cov_req", "cov_lreq", "cov_objs", "cov_api2",
      "pairs_DoRequest", "pairs_DoReply", "pairs_DoListRequest", "pairs_DoListReply", "pairs_CStart", "pairs_C1",
      "pairs_C10", "pairs_C11", "pairs_c12", "pairs_C13", "pairs_C2", "pairs_C3", "pairs_C8", "pairs_C6",
      "pairs_C7", "pairs_C4", "pairs_C5", "pairs_PVCStart", "pairs_PVCListedPVCs", "pairs_PVCHavePVCs",
      "pairs_PVCDone", "pairs_APIStart",
      "en_DoReply", "en_DoListReply", "en_APIStart", "states",
      "c13_ok", "c13_pvc", "c13_spec", "c7_ok", "c4_iter",
      "pvcl_ok", "pvcl_objs", "pvcl_objs_pvc", "pvcl_objs_spec",
      "create_exists", "force_iter", "force_setsz", "force_same",
      "get_iter", "get_iter_found", "get_setsz", "get_same",
      "del_setsz", "del_same", "upd_iter", "upd_nmatch", "upd_setsz", "upd_same",
      "list_setsz", "list_match"};
  return (i >= 0 && i < KC_COVER_N) ? kNames[i] : nullptr;
}

// the action whose label is pc (-1: none)
KC_HD int cover_label_action(int pc) {
  switch (pc) {
    case L_DoRequest: return A_DoRequest;   case L_DoReply: return A_DoReply;
    case L_DoListRequest: return A_DoListRequest; case L_DoListReply: return A_DoListReply;
    case L_CStart: return A_CStart; case L_C1: return A_C1; case L_C10: return A_C10;
    case L_C11: return A_C11; case L_c12: return A_c12; case L_C13: return A_C13;
    case L_C2: return A_C2; case L_C3: return A_C3; case L_C8: return A_C8;
    case L_C6: return A_C6; case L_C7: return A_C7; case L_C4: return A_C4;
    case L_C5: return A_C5; case L_PVCStart: return A_PVCStart;
    case L_PVCListedPVCs: return A_PVCListedPVCs; case L_PVCHavePVCs: return A_PVCHavePVCs;
    case L_PVCDone: return A_PVCDone;
    default: return -1;
  }
}

// the bits of x up to and including the lowest bit of m (all of x if m == 0):
// what an \E over x visits when it stops at its first element in m
KC_HD uint64_t cover_upto(uint64_t x, uint64_t m) {
  return m ? x & (((m & (~m + 1)) << 1) - 1) : x;
}

// U bits whose object has a spec / whose version vector holds actor a
template <class M>
constexpr uint64_t cover_spec_mask() {
  uint64_t r = 0;
  for (int u = 0; u < M::U; ++u)
    if ((u >> M::A) & 1) r |= 1ull << u;
  return r;
}
template <class M, int a>
constexpr uint64_t cover_read_mask() {
  uint64_t r = 0;
  for (int u = 0; u < M::U; ++u)
    if ((u >> a) & 1) r |= 1ull << u;
  return r;
}

// add(i, v): counter i of the state's vector grows by v (every index at most
// a few times per state; v < 2^13).
template <class M, class F>
KC_HD void cover_visit(const typename M::State& s, const Flags& f, F&& add) {
  constexpr int A = M::A, NS = M::NS;
  const uint64_t api = s.w[0] & M::UMASK;
  const uint32_t napi = (uint32_t)popc(api);
  add(CV_STATES, 1u);
  add(CV_COV_API, napi);
  add(CV_COV_API2, napi * napi);
  if (NS) add(CV_PAIRS + A_APIStart, (uint32_t)NS);
  bool pending = false;
  static_for<A>([&](auto AI) {
    constexpr int a = AI;
    const uint64_t w = M::template aw<a>(s);
    const int p = M::g(w, M::F_PC, M::B_PC);
    const int rqst = M::g(w, M::F_RQST, 2), lrst = M::g(w, M::F_LRST, 2);
    const bool rqp = M::g(w, M::F_RQP, 1), lrp = M::g(w, M::F_LRP, 1);
    const uint64_t objs = M::template objs<a>(s);
    const uint32_t nobjs = (uint32_t)popc(objs);
    if (rqp) add(CV_COV_REQ, 1u);
    if (lrp) {
      add(CV_COV_LREQ, 1u);
      add(CV_COV_OBJS, nobjs);
    }
    const int act = cover_label_action(p);
    if (act >= 0) add(CV_PAIRS + act, 1u);
    if (p == L_DoReply && rqst != ST_Pending) add(CV_EN_DOREPLY, 1u);
    if (p == L_DoListReply && lrst != ST_Pending) add(CV_EN_DOLISTREPLY, 1u);
    const bool ok = rqst == ST_Ok, lok = lrst == ST_Ok;
    if constexpr (M::is_client(a)) {
      switch (p) {
        case L_CStart: {                                        // :529-548, both branches of :529-531
          const uint32_t sr = (uint32_t)M::g(w, M::F_SR, 1);
          add(CV_B_CSTART_THEN, 1u + sr);
          add(CV_B_CSTART_ELSE, 1u - sr);
          break;
        }
        case L_C1: add((!ok && f.variant != 3) ? CV_B_C1_START : CV_B_C1_C10, 1u); break;
        case L_C11: add(!ok ? CV_B_C11_START : CV_B_C11_c12, 1u); break;
        case L_C13: {                                           // :590, IsUnboundPVC :444-446
          const int oc = M::g(w, M::F_RQOBJ, M::OBJB);
          const bool pvc = oc != 0 && M::oc_id(oc) == ID_PVC;
          const bool spec = M::oc_is_full(oc) && M::u_spec(M::oc_u(oc));
          if (ok) {
            add(CV_C13_OK, 1u);
            if (pvc) add(CV_C13_PVC, 1u);
            if (pvc && spec) add(CV_C13_SPEC, 1u);
          }
          add((!ok || (pvc && !spec)) ? CV_B_C13_START : CV_B_C13_C2, 1u);
          break;
        }
        case L_C3: add(!lok ? CV_B_C3_START : CV_B_C3_C8, 1u); break;
        case L_C8: add(objs == 0 ? CV_B_C8_C4 : CV_B_C8_C6, 1u); break;
        case L_C7:                                              // :632
          if (ok) add(CV_C7_OK, 1u);
          add((!ok || nobjs > 1) ? CV_B_C7_START : CV_B_C7_C4, 1u);
          break;
        case L_C4:                                              // :639, ObjectExists :410
          add(CV_C4_ITER, (uint32_t)popc(cover_upto(api, api & M::id_mask(ID_Secret))));
          break;
        default: break;
      }
    } else {
      if (p == L_PVCListedPVCs) {                               // :666-667
        const uint64_t pv = objs & M::id_mask(ID_PVC);
        if (lok) {
          add(CV_PVCL_OK, 1u);
          add(CV_PVCL_OBJS, nobjs);
          add(CV_PVCL_OBJS_PVC, (uint32_t)popc(pv));
          add(CV_PVCL_OBJS_SPEC, (uint32_t)popc(pv & cover_spec_mask<M>()));
        }
        add((!lok || M::unbound(objs) == 0) ? CV_B_PVCL_START : CV_B_PVCL_HAVE, 1u);
      }
    }
    // APIStart (:698-756), once per server: actor a's pending request ...
    if (NS && rqp && rqst == ST_Pending) {
      pending = true;
      const int oc = M::g(w, M::F_RQOBJ, M::OBJB);
      const uint64_t same = api & M::id_mask(oc ? M::oc_id(oc) : 0);
      const uint32_t nsame = (uint32_t)popc(same) * NS;
      const uint32_t it = (uint32_t)popc(cover_upto(api, same)) * NS;
      const uint32_t sz = napi * NS;
      switch (M::g(w, M::F_RQOP, 3)) {
        case OP_Create:
          add(CV_B_API_CREATE, (uint32_t)NS);
          if (same) add(CV_CREATE_EXISTS, (uint32_t)NS);
          break;
        case OP_Force:
          add(CV_B_API_FORCE, (uint32_t)NS);
          add(CV_FORCE_ITER, it);
          if (same) {
            add(CV_B_API_FORCE_REPLACE, (uint32_t)NS);
            add(CV_FORCE_SETSZ, sz);
            add(CV_FORCE_SAME, nsame);
          } else {
            add(CV_B_API_FORCE_CREATE, (uint32_t)NS);
          }
          break;
        case OP_Get:
          add(CV_B_API_GET, (uint32_t)NS);
          add(CV_GET_ITER, it);
          if (same) {
            add(CV_GET_ITER_FOUND, it);
            add(CV_GET_SETSZ, sz);
            add(CV_GET_SAME, nsame);
          } else {
            add(CV_B_API_GET_NOTFOUND, (uint32_t)NS);
          }
          break;
        case OP_Delete:
          add(CV_B_API_DELETE, (uint32_t)NS);
          add(CV_DEL_SETSZ, sz);
          add(CV_DEL_SAME, nsame);
          break;
        case OP_Update: {                                       // :733: IsVersionOf /\ HasRead, first match
          const uint64_t hit = same & cover_read_mask<M, a>();
          const bool applied = hit != 0 || (f.variant == 1 && same != 0);
          add(CV_B_API_UPDATE, (uint32_t)NS);
          add(applied ? CV_B_API_UPDATE_OK : CV_B_API_UPDATE_ERR, (uint32_t)NS);
          add(CV_UPD_ITER, (uint32_t)popc(cover_upto(api, hit)) * NS);
          add(CV_UPD_NMATCH, (uint32_t)popc(cover_upto(same, hit)) * NS);
          if (applied) {
            add(CV_UPD_SETSZ, sz);
            add(CV_UPD_SAME, nsame);
          }
          break;
        }
        default: add(CV_B_API_ASSERT, (uint32_t)NS); break;       // :740
      }
    }
    // ... and its pending list request (:745-753)
    if (NS && lrp && lrst == ST_Pending) {
      pending = true;
      add(CV_B_API_LIST, (uint32_t)NS);
      add(CV_LIST_SETSZ, napi * NS);
      add(CV_LIST_MATCH, (uint32_t)popc(api & M::kind_mask(M::g(w, M::F_LRK, 2))) * NS);
    }
  });
  if (pending) add(CV_EN_APISTART, (uint32_t)NS);
}

// The state's whole vector (host models and tests; kernels add into LDS).
template <class M>
KC_HD void cover_state(const typename M::State& s, const Flags& f, uint32_t out[KC_COVER_N]) {
  for (int i = 0; i < KC_COVER_N; ++i) out[i] = 0;
  cover_visit<M>(s, f, [&](int i, uint32_t v) { out[i] += v; });
}

}  // namespace kc
