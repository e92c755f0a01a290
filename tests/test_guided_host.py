"""The host layer of guided sampling without a device: the batch generator every runner shares (its --resume skip included) and the
attributes TwistedSampler and SumPotential dispatch their reports on (hasattr of `locate`, `describe`, `assign`)."""
import os


def _batches(tmp_path, present, **over):
    from genie2_amd.sample_unconditional import UnconditionalRunner
    outdir = str(tmp_path)
    os.makedirs(os.path.join(outdir, 'pdbs'), exist_ok=True)
    for index in present:
        open(os.path.join(outdir, 'pdbs', '7_{}.pdb'.format(index)), 'w').close()
    return list(UnconditionalRunner().batches(dict({'num_samples': 5, 'batch_size': 2}, **over), outdir, 7))


def test_batches_cover_num_samples_and_resume_skips_only_whole_written_batches(tmp_path):
    every = [(2, 0), (2, 2), (1, 4)]
    assert _batches(tmp_path / 'a', []) == every
    assert _batches(tmp_path / 'b', [0, 1], resume=True) == [(2, 2), (1, 4)]
    assert _batches(tmp_path / 'c', [0], resume=True) == every                 # half a batch: sampled again
    assert _batches(tmp_path / 'd', [0, 1, 2, 3, 4]) == every                  # without resume: whatever is there
    assert _batches(tmp_path / 'e', [0, 1], resume=False) == every
    assert _batches(tmp_path / 'f', [0, 1, 2, 3, 4], resume=True) == []


def _stand_in(**methods):
    """A plain callable potential with the given report methods."""
    def pot(x0, step):
        return x0.sum(dim=(1, 2))
    for name, fn in methods.items():
        setattr(pot, name, fn)
    return pot


def test_reports_are_dispatched_on_the_methods_a_potential_has():
    from genie2_amd import smc
    for name in ('locate', 'describe', 'assign', 'has_fit'):                    # a default would switch a report on for every potential
        assert not hasattr(smc._HipPotential, name)
    has = lambda cls: {n for n in ('locate', 'describe', 'assign') if hasattr(cls, n)}      # noqa: E731
    assert has(smc.MotifPotential) == {'locate'}
    assert has(smc.ShapePotential) == {'describe'}
    assert has(smc.SecStructPotential) == {'describe', 'assign'}
    for cls in (smc.MotifPotential, smc.ShapePotential, smc.SecStructPotential):
        assert has(object.__new__(cls)) == has(cls)                             # (an instance adds none of its own)
        assert issubclass(cls, smc._HipPotential) and all(hasattr(cls, n) for n in ('variance', '_checked', '_launch', '__call__'))
    shape_like = _stand_in(describe=lambda x: {'rog': 1.0})
    motif_like = _stand_in(locate=lambda x: {'best': 0})
    plain = _stand_in()
    assert has(shape_like) == {'describe'} and has(motif_like) == {'locate'} and has(plain) == set()
    assert has(smc.SumPotential(plain, motif_like)) == {'locate'}
    assert has(smc.SumPotential(motif_like, plain, plain)) == {'locate'}
    assert not hasattr(smc.SumPotential(plain, motif_like), 'describe')
    assert has(smc.SumPotential(plain, plain)) == set()
    both = smc.SumPotential(motif_like, shape_like)
    assert has(both) == {'locate', 'describe'} and both.describe(None) == {'rog': 1.0} and both.has_fit is True
    assert has(smc.SumPotential(shape_like, _stand_in(assign=lambda x: 0, describe=lambda x: {}))) == {'describe', 'assign'}


def test_one_autograd_function_serves_the_three_potentials():
    import torch
    from genie2_amd import smc
    fns = [v for v in vars(smc).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function)]
    assert len(fns) == 1
