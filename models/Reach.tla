---- MODULE Reach ----
\* User-defined invariants for models/Reach.cfg, in kubecheck.pred's language
\* (TLA+-flavoured predicates over KubeAPI.tla's variables; the file is read
\* by -defs, not by SANY).

\* at most one version each of the Secret and of the PVC is stored
StoreSmall == Cardinality(apiState) <= 2

\* a client that is done has nothing left to reconcile
DoneMeansReconciled ==
    \A c \in Clients : pc[c] = "C5" => ~shouldReconcile[c]

\* "can the client reach C5?", negated
ClientNeverDone == \A c \in Clients : pc[c] # "C5"

\* "... while the controller is done too?"
NeverBothDone == ~(pc["Client"] = "C5" /\ pc["PVCController"] = "PVCDone")
====
