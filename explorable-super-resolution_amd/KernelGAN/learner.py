"""The schedule of kernel estimation — the reference's codes/KernelGAN/learner.py (Learner).

Learning rates fall by 10 at every multiple of 750 iterations.  Once the bicubic loss has stayed below 0.4 for three iterations in a row,
lambda_bicubic falls by 100 at every multiple of 200 iterations (down to 5e-6), and the centralized and sparse terms are switched on when
it has passed 5e-3.  Everything the learner decides takes effect at a multiple of 200 or 750 only, so an engine that keeps the bicubic
loss of every iteration on the device can read 200 of them back at once and replay() them: the decisions are the same."""


class Learner:
    lambda_update_freq = 200
    bic_loss_to_start_change = 0.4
    lambda_bicubic_decay_rate = 100.
    update_l_rate_freq = 750
    update_l_rate_rate = 10.
    lambda_sparse_end = 5
    lambda_centralized_end = 1
    lambda_bicubic_min = 5e-6

    def __init__(self):
        self.bic_loss_counter = 0
        self.similar_to_bicubic = False
        self.insert_constraints = True

    def lr_falls(self, iteration):
        return iteration != 0 and iteration % self.update_l_rate_freq == 0

    def observe(self, iteration, loss_bicubic, lambdas):
        """One iteration's bookkeeping on `lambdas` (a dict with 'bicubic', 'centralized', 'sparse'); True when it changed them."""
        if iteration == 0:
            return False
        if not self.similar_to_bicubic:
            if loss_bicubic < self.bic_loss_to_start_change:
                if self.bic_loss_counter >= 2:
                    self.similar_to_bicubic = True
                else:
                    self.bic_loss_counter += 1
            else:
                self.bic_loss_counter = 0
        elif iteration % self.lambda_update_freq == 0 and lambdas['bicubic'] > self.lambda_bicubic_min:
            lambdas['bicubic'] = max(lambdas['bicubic'] / self.lambda_bicubic_decay_rate, self.lambda_bicubic_min)
            if self.insert_constraints and lambdas['bicubic'] < 5e-3:
                lambdas['centralized'] = self.lambda_centralized_end
                lambdas['sparse'] = self.lambda_sparse_end
                self.insert_constraints = False
            return True
        return False

    def replay(self, last_iteration, losses, lambdas):
        """The observe() calls of iterations last_iteration - len(losses) + 1 .. last_iteration from their recorded bicubic losses."""
        first = last_iteration - len(losses) + 1
        changed = False
        for i, loss in enumerate(losses):
            changed |= self.observe(first + i, float(loss), lambdas)
        return changed

    def update(self, iteration, gan):
        """The reference's per-iteration call on an object with optimizer_G / optimizer_D, loss_bicubic and the lambda_* attributes."""
        if self.lr_falls(iteration):
            for opt in (gan.optimizer_G, gan.optimizer_D):
                for group in opt.param_groups:
                    group['lr'] /= self.update_l_rate_rate
        lambdas = {'bicubic': gan.lambda_bicubic, 'centralized': gan.lambda_centralized, 'sparse': gan.lambda_sparse}
        if self.observe(iteration, float(gan.loss_bicubic), lambdas):
            gan.lambda_bicubic, gan.lambda_centralized, gan.lambda_sparse = lambdas['bicubic'], lambdas['centralized'], lambdas['sparse']
