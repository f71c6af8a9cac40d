"""Analyzers of finished (or running) runs -- counterpart of ``tc_gan/analyzers``.

`distdiff`: tuning curves generated from the parameters recorded at each generator step and their Kolmogorov-Smirnov
distance to the truth, for all selected steps in a few large GPU batches."""
