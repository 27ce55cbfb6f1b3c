#!/usr/bin/env python3
"""Generate tests/golden/best_agent_saver.json by EXECUTING the reference's own BestAgentSaver
(imitation_lib/utils/training.py:8-52), imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in
the build container only:

    python tests/golden/gen_best_agent_saver.py [--out FILE]

The saver is fed a recording stand-in for the agent: an object whose `epoch` the driver sets before every save() call (the
agent "as it is in that epoch") and whose save(path, full_save=) records the file's stem together with the `epoch` and
`J` the saved object carries.  The reference holds a deepcopy of the agent between the snapshot and the write, so the
recorded epoch is that of the snapshot, not of the write; the copies share one log through a class attribute.

For every n_epochs_save in N_EPOCHS_SAVE and every J sequence in SEQUENCES the driver calls save(agent, J) once per
entry and then save_curr_best_agent(), as the launcher does (examples/imitation_learning/experiment.py:65,67).  Stored
per case: n_epochs_save, the sequence's name and values, and `writes`, the list of

    dict(stem, epoch, J, call)

in the order written: the file name without its extension, the epoch and J the saved object carried (checked to be the
values the saver formatted into the name), and the index of the save() call during which the file was written
(len(sequence) for the final save_curr_best_agent()).  The sequences hold a tie, a decrease, a negative J
and values that differ only past the sixth decimal (distinct J, the same digits in the name).  No mushroom-rl piece is restated: the
class uses none.  The file regenerates byte for byte.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

N_EPOCHS_SAVE = (1, 3, -1, 500)
SEQUENCES = {
    "issue": [1.0, 0.5, 2.0, 2.0, 1.5, 3.0, -1.0, 0.0],
    "negative": [-2.0, -2.0, -3.5, -1.25, -1.25, 4.0, 0.25, -5.0, 6.0, 6.0, 5.0],
    "close": [0.1234561, 0.1234562, -0.1, 0.1234563, 0.0],
}


class RecordingAgent:
    log = []            # shared by the deep copies the saver makes

    def __init__(self):
        self.epoch, self.J = None, None

    def save(self, path, full_save=False):
        assert full_save is True
        RecordingAgent.log.append((os.path.splitext(os.path.basename(path))[0], self.epoch, self.J))


def run_case(saver_cls, n_epochs_save, seq):
    RecordingAgent.log = []
    saver = saver_cls("results", n_epochs_save=n_epochs_save)
    agent = RecordingAgent()
    writes = []

    def drain(call):
        for stem, epoch, J in RecordingAgent.log:
            # the name is formatted from the saver's own (epoch, J): they must be the saved copy's
            assert stem == "agent_epoch_%d_J_%f" % (epoch, J), (stem, epoch, J)
            writes.append(dict(stem=stem, epoch=epoch, J=J, call=call))
        RecordingAgent.log = []

    for call, J in enumerate(seq):
        agent.epoch, agent.J = call, J
        saver.save(agent, J)
        drain(call)
    saver.save_curr_best_agent()
    drain(len(seq))
    return writes


def main():
    out = os.path.join(HERE, "best_agent_saver.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    import importlib

    import _ref_stubs as stubs
    stubs.install()
    training = importlib.import_module("imitation_lib.utils.training")
    cases = []
    for name, seq in SEQUENCES.items():
        for n in N_EPOCHS_SAVE:
            writes = run_case(training.BestAgentSaver, n, seq)
            cases.append(dict(sequence=name, n_epochs_save=n, J=seq, writes=writes))
            print(f"{name} n_epochs_save={n}: " + (", ".join(w["stem"] for w in writes) or "nothing written"))
    with open(out, "w") as f:
        json.dump(dict(cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
