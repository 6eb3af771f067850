#!/usr/bin/env python
"""
Fitting a site-class codon model on the GPU: the p53 alignment under K = 3 omega classes in the
style of codeml's M3 -- MG94 with one kappa and one tree scale shared by the classes, an omega per
class, and the class weights through a softmax.  L-BFGS-B takes the value and the ANALYTIC
gradient in all seven parameters from ONE branch_expectations_mixture call per iteration:

  per class k three coefficient matrices, rate_parameter_coefs(Q_k, dQ_k / d log kappa),
  rate_parameter_coefs(Q_k, dQ_k / d log omega_k), and ones off the diagonal with diag(Q_k) on it
  (the direction Q_k itself: t d / d t);
  d / d log kappa    = sum over branches of edge_sums[:, 0]
  d / d log omega_k  = sum over branches of set_edge_sums[k, :, 1]
  d / d log scale    = sum over classes and branches of set_edge_sums[:, :, 2]
  d / d z_k          = class_sums[k] - c_k * (number of columns),  c = softmax(z)

The start-point gradient is printed next to forward differences taken through step_multi +
mixture_log_likelihoods, what examples/optimise_codon_lbfgs.py does with one extra rate set per
parameter.

    python examples/optimise_codon_site_classes.py [alignment.phylip tree.newick genetic.code.txt]

Defaults to the copies of the reference's data under tests/golden/p53/.
"""
import os
import sys

import numpy as np
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io      # noqa: E402

NT_FREQS = dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883)
K = 3
START = dict(kappa=2.0, omega=(0.05, 0.4, 1.5), scale=1.0, weights=(0.5, 0.3, 0.2))
EPS = 1e-6          # forward-difference step of the comparison (the parameters are logs / logits)


def codon_masks(code):
    """(transition, nonsynonymous) masks over the single-nucleotide changes of the code."""
    n = len(code)
    transitions = {('A', 'G'), ('G', 'A'), ('C', 'T'), ('T', 'C')}
    ts, ns = np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool)
    for sa, ra, ca in code:
        for sb, rb, cb in code:
            diff = [(x, y) for x, y in zip(ca, cb) if x != y]
            if len(diff) == 1:
                ts[sa, sb] = diff[0] in transitions
                ns[sa, sb] = ra != rb
    return ts, ns


def rates_and_derivatives(code, distn, ts, ns, kappa, omega):
    """MG94 scaled to expected rate 1 (io.mg94_from_code) with d Q / d log kappa and d Q / d log
    omega: the raw rates are multiplied by kappa on the transitions and by omega on the
    nonsynonymous changes, then everything is divided by the expected rate."""
    Q = io.mg94_from_code(code, kappa, omega, NT_FREQS)[0]
    out = []
    for mask in (ts, ns):
        dR = np.where(mask, Q, 0.0)                   # (already over the expected rate)
        dR -= np.diag(dR.sum(axis=1))
        d_rate = -float(np.dot(distn, np.diag(dR)))   # of the expected rate, relative
        out.append(dR - Q * d_rate)
    return Q, out[0], out[1]


def unpack(x):
    z = np.concatenate([[0.0], x[5:7]])
    c = np.exp(z - z.max())
    return np.exp(x[0]), np.exp(x[1:4]), np.exp(x[4]), c / c.sum()


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    aln = argv[1] if len(argv) > 1 else os.path.join(data, 'alignment.for.codeml.phylip')
    tree = argv[2] if len(argv) > 2 else os.path.join(data, 'p53S.const.tree')
    code_path = argv[3] if len(argv) > 3 else os.path.join(data, 'universal.code.txt')

    code = io.read_genetic_code(code_path)
    n = len(code)
    distn = io.mg94_from_code(code, 1.0, 1.0, NT_FREQS)[1]
    ts, ns = codon_masks(code)
    T, root, leaf_name_pairs = io.read_newick(open(tree).read())
    leaves, states = io.alignment_to_states(io.read_phylip(aln), code, leaf_name_pairs)
    ncols = states.shape[0]

    model = device.TreeModel(T, root, n)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state')          # once
    t0 = model.tree.branch_lengths()
    evaluations = [0]

    def rate_sets(x):
        kappa, omega, scale, c = unpack(x)
        parts = [rates_and_derivatives(code, distn, ts, ns, kappa, w) for w in omega]
        return np.array([p[0] for p in parts]), np.tile(scale * t0, (K, 1)), c, parts

    def objective(x):
        """-(log likelihood) and its gradient in (log kappa, log omega_1..3, log scale, z_2, z_3)
        from one branch_expectations_mixture call."""
        Q, t, c, parts = rate_sets(x)
        E = np.ones((K, 3, n, n))
        for k, (Qk, dkappa, domega) in enumerate(parts):
            E[k, 0] = device.rate_parameter_coefs(Qk, dkappa)
            E[k, 1] = device.rate_parameter_coefs(Qk, domega)
            np.fill_diagonal(E[k, 2], np.diag(Qk))
        model.set_rate_sets(Q, t=t)
        res = model.branch_expectations_mixture(batch, E, c, per_site=False)
        if res.status.any():
            raise SystemExit('%d columns of zero likelihood' % int((res.status & 1).sum()))
        evaluations[0] += 1
        g = np.concatenate([[res.edge_sums[:, 0].sum()], res.set_edge_sums[:, :, 1].sum(axis=1),
                            [res.set_edge_sums[:, :, 2].sum()],
                            (res.class_sums - c * ncols)[1:]])
        return -float(res.log_likelihoods.sum()), -g

    def value_by_step_multi(x):
        Q, t, c, _ = rate_sets(x)
        model.set_rate_sets(Q, t=t)
        model.step_multi(batch, recompute_transitions=False)
        return -float(model.mixture_log_likelihoods(batch, c)[0].sum())

    x0 = np.concatenate([[np.log(START['kappa'])], np.log(START['omega']), [np.log(START['scale'])],
                         np.log(START['weights'])[1:] - np.log(START['weights'][0])])
    f0, g0 = objective(x0)
    base = value_by_step_multi(x0)
    fd = np.array([(value_by_step_multi(x0 + EPS * np.eye(7)[j]) - base) / EPS for j in range(7)])
    print('%d taxa, %d codon columns, %d classes; start %.6f (step_multi: %.6f)'
          % (len(leaves), ncols, K, -f0, -base))
    names = ['log kappa'] + ['log omega_%d' % (k + 1) for k in range(K)] + ['log scale', 'z_2', 'z_3']
    print('gradient of the log likelihood at the start: analytic (one call) | forward differences '
          '(seven more step_multi)')
    for name, a, b in zip(names, -g0, -fd):
        print('  %-12s %+.9e | %+.9e' % (name, a, b))
    assert np.allclose(g0, fd, rtol=1e-3, atol=1e-3 * np.abs(g0).max())
    bounds = [(-3.0, 3.0)] + [(-7.0, 3.0)] * K + [(-3.0, 3.0)] + [(-8.0, 8.0)] * 2
    fit = scipy.optimize.minimize(objective, x0, jac=True, method='L-BFGS-B', bounds=bounds,
                                  options=dict(maxiter=500, ftol=1e-12, gtol=1e-6))
    kappa, omega, scale, c = unpack(fit.x)
    print('%s after %d iterations, %d evaluations (each: one set_rate_sets + one '
          'branch_expectations_mixture)' % ('converged' if fit.success else 'stopped: %s' % fit.message,
                                            fit.nit, evaluations[0]))
    print('log likelihood %.6f (start %.6f); largest |gradient| %.2e'
          % (-fit.fun, -f0, np.abs(fit.jac).max()))
    print('kappa %.4f, tree scale %.4f; omega classes %s with weights %s'
          % (kappa, scale, ', '.join('%.4f' % w for w in omega), ', '.join('%.4f' % w for w in c)))
    post, _ = model.class_posteriors(batch, c)
    top = int(np.argmax(omega))
    print('%d columns with posterior > 0.95 for the class of the largest omega'
          % int((post[:, top] > 0.95).sum()))
    assert -fit.fun >= -f0
    batch.close()
    model.close()


if __name__ == '__main__':
    main(sys.argv)
