"""Run by tests/test_dropin_binding.py in its own process (it installs in-memory `models` / `data` packages and sets
sys.argv): applies the reference-side binding of INTEGRATION.md section 1 -- the code blocks of that file, verbatim --
to a replay of the reference's plugin loader and option gather, and reports what the loader finds.

The reference's side comes from tests/golden/dropin.json (recorded from the reference by tests/golden/make_dropin.py):
the argparse actions of its TrainOptions, the dataset setter's additions, the fields parse() sets beyond the parser and
the command line.  The loader follows the contract of models/__init__.py:25-67: `models.<name>_model` is imported and
the class whose lower-cased name is `<name without underscores>model` and that subclasses models.BaseModel is the
model (the last such name in the module's namespace: the reference's loop keeps the last match); the option setter is
that class's modify_commandline_options.  Options recorded with the reference's util.str2bool type are rebuilt with the
package's str2bool (dfmir_amd.registration_model), which accepts the same spellings; the recorded command line passes
none of them.  The gather is options/base_options.py:75-110 and 141-164: parse the known arguments, apply the model's
setter, parse again, apply the dataset's setter, parse."""
import abc
import argparse
import ast
import importlib
import json
import os
import re
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def integration_blocks():
    """The python code blocks of INTEGRATION.md section 1, in order."""
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    sec = text.split("## 1.")[1].split("## 2.")[0]
    return re.findall(r"```python\n(.*?)```", sec, flags=re.S)


def recorded_parser(rec, str2bool):
    """The reference TrainOptions parser, rebuilt from the recorded actions (+ the dataset setter's)."""
    types_ = {None: None, "int": int, "float": float, "str": str, "str2bool": str2bool}
    parser = argparse.ArgumentParser()
    for a in rec["actions"] + rec["dataset_actions"]:
        kw = {"dest": a["dest"], "default": a["default"]}
        if a["kind"] == "store":
            kw["type"] = types_[a["type"]]
            if a["nargs"] is not None:
                kw["nargs"] = a["nargs"]
            if a["const"] is not None:
                kw["const"] = a["const"]
            if a["choices"] is not None:
                kw["choices"] = a["choices"]
        else:
            kw["action"] = a["kind"]
        parser.add_argument(*a["option_strings"], **kw)
    return parser


def main():
    rec = json.load(open(os.path.join(REPO, "tests", "golden", "dropin.json")))
    blocks = integration_blocks()
    model_block = [b for b in blocks if "REGISTRATIONModel" in b][0]
    register_block = [b for b in blocks if "BaseModel.register" in b][0]
    factory_block = [b for b in blocks if "define_G" in b][0]

    # the reference's `models` package as the binding sees it: an abstract BaseModel, the loader's two lookups
    assert rec["base_model_is_abc"]
    models = types.ModuleType("models")
    models.__path__ = []
    models.BaseModel = abc.ABCMeta("BaseModel", (object,), {})

    def find_model_using_name(name):
        lib = importlib.import_module("models.%s_model" % name)
        want = name.replace("_", "").lower() + "model"
        hits = [c for k, c in vars(lib).items()
                if k.lower() == want and isinstance(c, type) and issubclass(c, models.BaseModel)]
        if not hits:
            raise ImportError("no subclass of BaseModel named %s in models.%s_model" % (want, name))
        return hits[-1]

    models.find_model_using_name = find_model_using_name
    models.get_option_setter = lambda name: find_model_using_name(name).modify_commandline_options
    sys.modules["models"] = models
    # `models/registration_model.py -- replace the body with:` the re-export
    mod = types.ModuleType("models.registration_model")
    mod.__file__ = "<INTEGRATION.md section 1>"
    exec(compile(model_block, mod.__file__, "exec"), mod.__dict__)
    sys.modules["models.registration_model"] = mod
    models.registration_model = mod
    # `models/__init__.py, after the BaseModel import`
    exec(compile(register_block, "<INTEGRATION.md section 1>", "exec"), models.__dict__)
    ns = {}
    exec(compile(factory_block, "<INTEGRATION.md section 1>", "exec"), ns)   # the factory re-exports import cleanly

    out = {}
    cls = models.find_model_using_name("registration")
    import dfmir_amd.registration_model as hip
    out["found_hip_class"] = cls is hip.REGISTRATIONModel
    out["option_setter_is_hip"] = models.get_option_setter("registration") == hip.REGISTRATIONModel.modify_commandline_options

    # TrainOptions().parse() through the reference's two-pass gather (the setters read sys.argv themselves)
    sys.argv = ["train.py"] + rec["argv"]
    parser = recorded_parser(rec, hip.str2bool)
    opt, _ = parser.parse_known_args()
    parser = models.get_option_setter(opt.model)(parser, rec["is_train"])
    opt, _ = parser.parse_known_args()
    parser.set_defaults(**rec["dataset_defaults"])
    opt = parser.parse_args()
    for f in rec["set_by_parse"]:
        assert f == "isTrain", f
        opt.isTrain = rec["is_train"]
    out["opt_model"] = opt.model
    out["nce_idt"], out["lambda_NCE"], out["pool_size"] = bool(opt.nce_idt), float(opt.lambda_NCE), int(opt.pool_size)
    # every `opt.<field>` the package reads (not through getattr) must exist on the reference's parsed options
    missing, read = [], set()
    pkg = os.path.join(REPO, "dfmir_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py") or fn in ("options.py", "train.py", "test.py"):   # (those BUILD their options, they do not consume the reference's)
            continue
        for node in ast.walk(ast.parse(open(os.path.join(pkg, fn)).read())):      # attribute READS in code, not prose
            if not (isinstance(node, ast.Attribute) and isinstance(node.ctx, ast.Load)):
                continue
            v = node.value
            is_opt = (isinstance(v, ast.Name) and v.id == "opt") or (
                isinstance(v, ast.Attribute) and v.attr == "opt" and isinstance(v.value, ast.Name) and v.value.id == "self")
            if is_opt:
                read.add(node.attr)
                if not hasattr(opt, node.attr):
                    missing.append("%s:%s" % (fn, node.attr))
    out["fields_read"] = sorted(read)
    out["missing_fields"] = sorted(set(missing))
    out["factories"] = sorted(k for k in ns if not k.startswith("__"))
    print("DROPIN_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
