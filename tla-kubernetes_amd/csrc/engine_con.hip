// engine_con.hip — the single-GPU engine under constraints
// (kc_model_config.constraint_stored, constraint_inflight, action_constraints;
// DESIGN.md section 4.11): EngineT<ConModel<..>> for the models built with
// constraints, instantiated from engine.hip's text in a translation unit of
// its own, so the plain instantiations compile exactly as before and the
// units build in parallel.
#define KC_ENGINE_CON_TU 1
#include "engine.hip"
