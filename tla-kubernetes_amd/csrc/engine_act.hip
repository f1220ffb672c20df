// engine_act.hip — the single-GPU engine under action properties
// (kc_model_config.action_properties):
// EngineT<ActModel<..>> for the models built with them, instantiated from
// engine.hip's text in a translation unit of its own, so the plain, symmetric
// and constrained instantiations compile exactly as before and the units
// build in parallel.
#define KC_ENGINE_ACT_TU 1
#include "engine.hip"
