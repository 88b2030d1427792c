"""Worker of tests/multiproc/test_binarize_multiproc.py: ``vae-hpo.py``'s own
``main`` with the command line given after the script name; afterwards every
rank prints ``RESULT <json>`` with a digest of the parameters and Adam moments
of the trainer its trial built.
"""
import faulthandler
import hashlib
import importlib.util
import json
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from multidisttorch_amd.hpo import runner

    made = []
    real = runner._make_trainer

    def spy(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]

    runner._make_trainer = spy
    spec = importlib.util.spec_from_file_location("vae_hpo_main", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(sys.argv[1:])
    tr = made[-1]
    h = hashlib.sha256()
    for t in (tr.params, tr.exp_avg, tr.exp_avg_sq):
        h.update(t.detach().cpu().numpy().tobytes())
    print("RESULT " + json.dumps(dict(rank=int(os.environ.get("RANK", "0")), step=tr.step_count,
                                      digest=h.hexdigest())), flush=True)


if __name__ == "__main__":
    main()
