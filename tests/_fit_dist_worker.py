"""Worker of tests/test_fit_host.py::test_item_msq_refuses_two_ranks_in_the_wording_of_item_fit: item_msq on a gloo group of two,
through the model class and on the engine, and item_fit through the model class; writes the names of the three exceptions and
their messages."""
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
    y = torch.from_numpy((np.random.RandomState(3).uniform(size=(20, 8)) < 0.5).astype(np.uint8))
    m = vi.VIRT(data=y[rank * 10:rank * 10 + 10], model="irt_2pl", sample_size_global=20, gid0=rank * 10,
                group=torch.distributed.group.WORLD, backend=OracleBackend())
    names, messages = [], []
    for call in (m.item_msq, m.engine.item_msq, m.item_fit):
        try:
            call()
            names.append("none")
            messages.append("")
        except Exception as e:                           # noqa: BLE001  (the name and the message are what the test reads)
            names.append(type(e).__name__)
            messages.append(" ".join(str(e).split()))
    with open(out_path + ".%d" % rank, "w") as f:
        f.write("\n".join([" ".join(names)] + messages) + "\n")
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
