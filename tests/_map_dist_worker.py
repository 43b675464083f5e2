"""Worker of tests/test_map_host.py::test_two_ranks_refuse: fit_em(prior=) on a gloo group of two, through the model class and on
the engine; writes the names of the two exceptions."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.map_cases import MapOracleBackend            # noqa: E402
from vipsy_amd import vi                                # noqa: E402


def main():
    out_path = sys.argv[1]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    torch.distributed.init_process_group(backend="gloo", rank=rank, world_size=world)
    y = torch.from_numpy((np.random.RandomState(3).uniform(size=(20, 8)) < 0.5).astype(np.uint8))
    m = vi.VIRT(data=y[rank * 10:rank * 10 + 10], model="irt_3pl", sample_size_global=20, gid0=rank * 10,
                group=torch.distributed.group.WORLD, backend=MapOracleBackend())
    names = []
    for call in (m.fit_em, m.engine.fit_em):
        try:
            call(max_iter=1, prior={"c": (-1.4, 1.0)})
            names.append("none")
        except Exception as e:                           # noqa: BLE001  (the name is what the test reads)
            names.append(type(e).__name__)
    with open(out_path + ".%d" % rank, "w") as f:
        f.write(" ".join(names))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
