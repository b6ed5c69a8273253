"""Generate tests/golden/dropin.json: what the REFERENCE's option machinery hands a model plugin.

Runs ONLY next to the reference tree (imports it through the shims of make_golden.py).  Records, as data:
  * the argparse actions TrainOptions.initialize() defines (options/base_options.py, options/train_options.py) --
    option strings, dest, default, type, nargs / const / choices;
  * what the dataset option setter of the parsed dataset_mode adds or re-defaults (options/base_options.py:100-103);
  * the fields parse() sets beyond the parser's dests (options/base_options.py:141-164);
  * whether models.BaseModel is an abstract base class (the INTEGRATION.md binding calls BaseModel.register);
  * the command line of make_golden.ref_options (temporary directories as placeholders).
tests/dropin_probe.py replays the reference's two-pass gather on these records with the INTEGRATION.md section 1 binding.
No reference source is stored: names, defaults and types only.

    python tests/golden/make_dropin.py
"""
import abc
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as MG  # noqa: E402

ARGV = ["--dataroot", "DATAROOT", "--gpu_ids", "-1", "--checkpoints_dir", "CHECKPOINTS", "--name", "g",
        "--batch_size", "2", "--crop_size", "64", "--load_size", "64", "--ngf", "8", "--CUT_mode", "CUT", "--no_flip"]


def _type_name(t):
    if t is None:
        return None
    if t in (int, float, str):
        return t.__name__
    if getattr(t, "__name__", "") == "str2bool":
        return "str2bool"
    raise ValueError("unrecorded option type %r" % (t,))


def _actions(parser):
    out = []
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        kind = {argparse._StoreTrueAction: "store_true", argparse._StoreFalseAction: "store_false",
                argparse._StoreAction: "store"}[type(a)]
        out.append({"option_strings": list(a.option_strings), "dest": a.dest, "kind": kind, "default": a.default,
                    "type": _type_name(a.type), "nargs": a.nargs, "const": a.const,
                    "choices": list(a.choices) if isinstance(a.choices, (list, tuple)) else a.choices})
    return out


def main():
    MG.install_shims()
    import data
    import models
    from options.train_options import TrainOptions
    o = TrainOptions()
    base = o.initialize(argparse.ArgumentParser())
    actions = _actions(base)
    opt, _ = base.parse_known_args(ARGV)
    # the dataset setter on a parser of its own: the actions it adds and the defaults it rewrites
    ds = data.get_option_setter(opt.dataset_mode)(o.initialize(argparse.ArgumentParser()), True)
    known = {a["dest"]: a for a in actions}
    ds_actions = [a for a in _actions(ds) if a["dest"] not in known]
    ds_defaults = {a["dest"]: a["default"] for a in _actions(ds) if a["dest"] in known and a["default"] != known[a["dest"]]["default"]}
    # what parse() adds beyond the dests: run it on the reference's own model setter (its options are not recorded)
    # (parse() writes its option file under --checkpoints_dir: temporary directories stand in for the placeholders)
    tmp = tempfile.mkdtemp(prefix="dfmir_dropin_")
    argv0 = sys.argv
    sys.argv = ["train.py"] + [tmp if a in ("DATAROOT", "CHECKPOINTS") else a for a in ARGV]
    full = TrainOptions().parse()
    p = TrainOptions()
    p.gather_options()
    sys.argv = argv0
    dests = {a.dest for a in p.parser._actions}
    rec = {"argv": ARGV, "is_train": True, "actions": actions, "dataset_actions": ds_actions,
           "dataset_defaults": ds_defaults, "set_by_parse": sorted(set(vars(full)) - dests),
           "base_model_is_abc": isinstance(models.BaseModel, abc.ABCMeta)}
    path = os.path.join(HERE, "dropin.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote dropin.json: %d actions, %d dataset actions, set by parse(): %s"
          % (len(actions), len(ds_actions), rec["set_by_parse"]))


if __name__ == "__main__":
    main()
