"""Worker of tests/test_pop_host.py::test_fit_population_refuses_two_ranks: fit_population on a gloo group of two, through the model
class and on the engine; writes the names of the two exceptions, whether a population was stored, and the messages."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.oracle_backend import OracleBackend          # noqa: E402
from vipsy_amd import vi                                # noqa: E402


def main():
    out_path = sys.argv[1]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    torch.distributed.init_process_group(backend="gloo", rank=rank, world_size=world)
    rng = np.random.RandomState(3)
    y = torch.from_numpy((rng.uniform(size=(20, 8)) < 0.5).astype(np.uint8))
    x = rng.normal(size=(10, 2))
    m = vi.VIRT(data=y[rank * 10:rank * 10 + 10], model="irt_2pl", sample_size_global=20, gid0=rank * 10,
                group=torch.distributed.group.WORLD, backend=OracleBackend())
    names, messages = [], []
    for call in (m.fit_population, m.engine.fit_population):
        try:
            call(x)
            names.append("none")
            messages.append("")
        except Exception as e:                           # noqa: BLE001  (the name and the message are what the test reads)
            names.append(type(e).__name__)
            messages.append(" ".join(str(e).split()))
    names.append("population=%s" % (m.engine.population,))
    with open(out_path + ".%d" % rank, "w") as f:
        f.write("\n".join([" ".join(names)] + messages) + "\n")
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
