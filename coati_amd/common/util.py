"""coati.common.util (coati/common/util.py) without its cloud-storage side: small host helpers, batch_indexable among them (the
reference's notebooks embed ChEMBL in slices of 1024 with it)."""
import datetime
import gc
import json
import multiprocessing as mp
import os
import shutil
import signal
import sys
from itertools import product

import numpy as np
import torch


def dir_or_file_exists(d):
    return os.path.exists(d)


def tensor_of_dict_of_lists(d: dict):
    """{k: [v0, v1, ...], ...} -> one dict per element of the Cartesian product of the value lists (keys in d's order)."""
    keys = list(d.keys())
    return [dict(zip(keys, combo)) for combo in product(*d.values())]


def colored_background(r: int, g: int, b: int, text):
    """text on a 24-bit ANSI background colour (r, g, b in 0..255)"""
    return "\033[48;2;%d;%d;%dm%s\033[0m" % (r, g, b, text)


def batch_indexable(iterable, n=128):
    """Yields consecutive slices iterable[i : i + n] of an indexable sequence (the last one may be shorter)."""
    total = len(iterable)
    for start in range(0, total, n):
        yield iterable[start:min(start + n, total)]


class NpEncoder(json.JSONEncoder):
    """json encoder that also takes numpy scalars, numpy arrays and torch tensors"""

    def default(self, obj):
        if isinstance(obj, np.integer):
            return int(obj)
        if isinstance(obj, np.floating):
            return float(obj)
        if isinstance(obj, (np.ndarray, torch.Tensor)):
            return obj.tolist()
        return super().default(obj)


def json_valid_dict(obj):
    return json.loads(json.dumps(obj, cls=NpEncoder))


def utc_epoch_now():
    return datetime.datetime.now().replace(tzinfo=datetime.timezone.utc).timestamp()


def makedir(path: str, isfile: bool = False):
    """Creates the directory `path` (isfile: the directory that holds the file `path`)."""
    d = os.path.dirname(path) if isfile else path
    if d:
        os.makedirs(d, exist_ok=True)


def rmdir(path: str):
    """Removes a directory tree; a failure is printed, not raised."""
    try:
        shutil.rmtree(path)
    except Exception as ex:
        print("rmdir failure", ex)


class OnlineEstimator:
    """Running mean / variance (Welford) without storing the samples.  Built from the first sample; each call adds one and returns
    (mean, unbiased variance)."""

    def __init__(self, x_):
        self.n = 1
        self.mean = x_ * 0.0
        self.m2 = x_ * 0.0
        self._add(x_)

    def _add(self, x_):
        d = x_ - self.mean
        self.mean += d / self.n
        self.m2 += d * (x_ - self.mean)

    def __call__(self, x_):
        self.n += 1
        self._add(x_)
        return self.mean, self.m2 / (self.n - 1)


def get_all_allocated_torch_tensors():
    """every live object the garbage collector knows that is a tensor or holds one in .data (memory-leak hunting)"""
    found = []
    for obj in gc.get_objects():
        try:
            if torch.is_tensor(obj) or (hasattr(obj, "data") and torch.is_tensor(obj.data)):
                found.append(obj)
        except Exception:
            pass
    return found


def records_mp(recs, func, args=None, n=None):
    """func(chunk, *args) over chunks of recs in a process pool; the per-chunk lists are concatenated in order."""
    n = min(mp.cpu_count(), len(recs)) if n is None else n
    args = tuple() if args is None else args
    count = len(recs)
    with mp.Pool(processes=n) as pool:
        parts = pool.starmap(func, [(chunk, *args) for chunk in batch_indexable(recs, n)])
    out = [r for part in parts for r in part]
    assert len(out) == count
    return out


def execute_with_timeout(method, args, timeout):
    """method(*args), or None when it has not returned after `timeout` seconds (SIGALRM: main thread only)."""
    def on_alarm(signum, frame):
        raise TimeoutError("Execution timed out")

    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(timeout)
    result = None
    try:
        result = method(*args)
    except TimeoutError:
        pass
    finally:
        signal.alarm(0)
    return result


def get_tnet_dir():
    """the directory that holds the package (the repository root in a source checkout)"""
    return os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dicts_to_keyval(list_of_dicts, key: str, value: str):
    return {d[key]: d[value] for d in list_of_dicts}


def query_yes_no(question, default=None):
    """Asks a yes / no question on stdin until it gets an answer; default ("yes", "no" or None) is taken on an empty line."""
    answers = {"yes": True, "y": True, "ye": True, "no": False, "n": False}
    prompts = {None: " [y/n] ", "yes": " [Y/n] ", "no": " [y/N] "}
    if default not in prompts:
        raise ValueError("invalid default answer: '%s'" % default)
    while True:
        sys.stdout.write(question + prompts[default])
        choice = input().lower()
        if default is not None and choice == "":
            return answers[default]
        if choice in answers:
            return answers[choice]
        sys.stdout.write("Please respond with 'yes' or 'no' (or 'y' or 'n').\n")
