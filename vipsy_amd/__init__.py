"""vipsy_amd: MI355X-native ELBO-gradient engine behind the vi.py model-class surface: fit(), and after it score() /
marginal_loglik() (grid posteriors: EAP, PSD, marginal log-likelihood, attribute classification)."""
__all__ = ["engine", "vi", "_hip"]
