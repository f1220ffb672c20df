---- MODULE Eventually ----
\* User-defined temporal properties for models/Eventually.cfg: state predicates
\* in kubecheck.pred's language under one temporal shape each, P ~> Q,
\* [](P => <>Q), []<>Q or <>Q (the file is read by -defs, not by SANY).

\* a client that is done does not stay unreconciled for ever
DoneIsReconciled == pc["Client"] = "C5" ~> ~shouldReconcile["Client"]

\* every behaviour gets the controller past its start label: violated under
\* WF_vars(Next), which lets the controller starve; holds under -fairness process
EventuallyListed == <>(pc["PVCController"] # "PVCStart")

\* once at C2 the client gets back to its start label
C2Restarts == pc["Client"] = "C2" ~> pc["Client"] = "CStart"

\* the same in the box-diamond spelling
C2RestartsBoxed == [](pc["Client"] = "C2" => <>(pc["Client"] = "CStart"))

\* the build-defined ClientRestarts, spelled out
ClientRestartsSpelled == []<>(pc["Client"] = "CStart")
====
