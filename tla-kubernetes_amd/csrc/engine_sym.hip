// engine_sym.hip — the single-GPU engine under symmetry reduction
// (kc_model_config.symmetry): EngineT<SymModel<..>> for the
// models with a non-trivial permutation group, instantiated from engine.hip's
// unchanged text in a translation unit of its own, so the plain
// instantiations compile exactly as before and the two build in parallel.
#define KC_ENGINE_SYM_TU 1
#include "engine.hip"
