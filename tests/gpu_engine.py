"""Engines for the GPU tests that compare with tests/score_ref.py: a Config over made-up triples holding given tables."""
import numpy as np


def make_engine(model, E, R, De, Dr, params, train=None):
    """A Config over made-up training triples (init_from_arrays) holding the given tables."""
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_work_threads(1)
    con.set_dimension(De)
    if model == "transr":
        con.set_ent_dimension(De); con.set_rel_dimension(Dr)
    if train is None:
        hh = np.arange(40) % E
        train = (hh, (hh + 1) % E, hh % R)
    con.init_from_arrays(E, R, *train)
    con.set_model_and_session(getattr(pkg, {"transe": "TransE", "transh": "TransH", "transd": "TransD", "transr": "TransR"}[model]))
    con.set_parameters(params)
    return con
