"""A ResNet replica trains from an image dataset directory on an MI355X: the input
kernel feeds the step from a resident and from a staged dataset, the validation
pass runs, and a resumed job continues with the batch an uninterrupted one reads."""
import math
import os
import re
import sys

import pytest
import torch

from kubeflow_controller_amd.api import v1alpha1
from kubeflow_controller_amd.cli.controller_main import Node
from kubeflow_controller_amd.cli.kfctl import describe_tfjob, wait_for_phase
from kubeflow_controller_amd.models.imagenet import ImageDataset, write_synthetic_dataset
from kubeflow_controller_amd.store import ObjectStore

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = [sys.executable, os.path.join(ROOT, "examples", "workdir", "train.py")]
N, SIZE = 96, 40


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("images"))
    write_synthetic_dataset(d, N, SIZE, 10, seed=2, n_val=20)
    return d


@pytest.fixture
def node(tmp_path):
    st = ObjectStore()
    n = Node(st, kubelet=True, root_dir=str(tmp_path), num_gpus=1, resync=30, kubelet_backoff=0.5,
             extra_env={"PYTHONPATH": ROOT}).start()
    yield st, n, str(tmp_path)
    n.shutdown()


def _run(node, name, args, model_dir=None):
    st, n, root = node
    c = {"name": "trainer", "command": TRAIN + args, "resources": {"limits": {"amd.com/gpu": 1}}}
    spec = {"tfReplicaSpec": [{"replicas": 1, "tfReplicaType": "Local",
                               "template": {"spec": {"containers": [c], "restartPolicy": "OnFailure"}}}]}
    if model_dir:
        spec["modelDir"] = model_dir
    st.create(v1alpha1.TFJob.from_json({"apiVersion": v1alpha1.API_VERSION, "kind": "TFJob",
                                        "metadata": {"name": name}, "spec": spec}))
    j = wait_for_phase(st, "default", name, {"Succeeded", "Failed"}, 300)
    pod = next(p for p in st.list("Pod") if p.metadata.name.startswith(name))
    d = os.path.join(root, f"default_{pod.metadata.name}")
    out = "".join(open(os.path.join(d, f)).read() for f in os.listdir(d) if f.endswith(".log"))
    assert j.status.phase == "Succeeded", describe_tfjob(st, "default", name) + out
    return out


def _args(data_dir, *extra):
    return ["--model", "resnet_tiny", "--data_dir", data_dir, "--batch_size", "8", "--train_steps", "4",
            "--optimizer", "sgd", "--learning_rate", "0.05", "--momentum", "0.9", "--log_every", "1", *extra]


@pytest.mark.parametrize("mode, extra", [("resident", []), ("staged", ["--data_resident_gb", "0"])])
def test_gpu_replica_trains_on_a_dataset_directory(node, data_dir, mode, extra):
    out = _run(node, f"rn-data-{mode}", _args(data_dir, *extra))
    assert "device cuda:0" in out
    assert f"data ready: {data_dir}, {N} training images {SIZE}x{SIZE}, 20 validation images" in out
    assert ("training images resident on cuda:0" if mode == "resident" else "training images staged per batch") in out
    loss = float(re.search(r"Final loss: (\S+)", out).group(1))
    m = re.search(r"Validation: top-1 accuracy = (\S+), cross entropy = (\S+) over 20 images", out)
    assert m, out
    assert math.isfinite(loss) and math.isfinite(float(m.group(2))) and 0.0 <= float(m.group(1)) <= 1.0


def test_gpu_resumed_job_reads_the_batch_an_uninterrupted_one_would(node, data_dir, tmp_path):
    model_dir = str(tmp_path / "ckpt")
    _run(node, "rn-data-a", _args(data_dir)[:6] + ["--train_steps", "2"] + _args(data_dir)[8:], model_dir)
    out = _run(node, "rn-data-b", _args(data_dir), model_dir)
    assert "resumed from" in out and "at global step 2" in out
    assert "next batch: step 2" in out  # the replica hands the restored step to the dataset
    d = torch.device("cuda")
    straight = ImageDataset(data_dir, (32, 32), seed=1234).to(d)
    for _ in range(2):
        straight.next_batch(8)
    a = straight.next_batch(8)
    resumed = ImageDataset(data_dir, (32, 32), seed=1234, data_resident_gb=0).to(d)
    resumed.set_step(2)
    b = resumed.next_batch(8)
    c = ImageDataset(data_dir, (32, 32), seed=1234).batch_at(2, 8)  # the CPU path, fp32
    assert a[0].dtype == torch.bfloat16 and a[0].is_cuda
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[1].cpu(), c[1])
    assert torch.allclose(a[0].float().cpu(), c[0], rtol=2 ** -7, atol=1e-5)
    resumed.close()
