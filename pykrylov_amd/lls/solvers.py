import numpy as np

from .. import _lib
from ..generic import KrylovMethod, DeviceRun, as_f64_vector, resolve_precon

__docformat__ = 'restructuredtext'

_STATUS = {0: 'solution is zero', 1: 'residual small', 2: 'residual small', 4: 'residual small',
           5: 'residual small', 3: 'ill-conditioned operator', 6: 'ill-conditioned operator',
           7: 'max iterations', 8: 'direct error small'}


class _LlsBase(KrylovMethod):
    """Shared device glue of the four least-squares solvers."""

    kind = None

    def __init__(self, A, **kwargs):
        KrylovMethod.__init__(self, A, **kwargs)
        self.A = A
        self.x = None
        self.var = None
        self.itn = 0
        self.istop = 0
        self.optimal = False
        self.resids = []
        self.normal_eqns_resids = []
        self.dir_errors_window = []
        self.iterates = []
        self.precon_route = {'M': 'none', 'N': 'none'}       # how the last solve applied M and N (see generic.resolve_precon)
        self.msg = ['The exact solution is  x = 0                              ',
                    'Ax - b is small enough, given atol, btol                  ',
                    'The least-squares solution is good enough, given atol     ',
                    'The estimate of cond(Abar) has exceeded conlim            ',
                    'Ax - b is small enough for this machine                   ',
                    'The least-squares solution is good enough for this machine',
                    'Cond(Abar) seems to be too large for this machine         ',
                    'The iteration limit has been reached                      ',
                    'The truncated direct error is small enough, given etol    ']

    def _trnc_dir_err(self, res):
        """trncDirErr of the last pass for the `show` summaries: the window's ratio trnc / sqrt(xNrgNorm2) the device
        records (lsqr.py:310-318), times sqrt(xNrgNorm2); 0 while the window is not full (the reference's initial value)."""
        d = self.dir_errors_window
        return float(d[-1]) * float(np.sqrt(res.aux[3])) if len(d) and np.isfinite(d[-1]) else 0.0

    def _run(self, rhs, itnlim, damp, atol, btol, conlim, M, N, kwargs):
        A = self._device_operator()
        m, n = A.shape
        # M and N: the reference calls them as functions, `u = M(Mu)`, `v = N(Nv)` (lsqr.py:190,202)
        name = self.__class__.__name__
        sides = (resolve_precon(M, m, 'M', name), resolve_precon(N, n, 'N', name))
        self.precon_route = {'M': sides[0][0], 'N': sides[1][0]}
        if kwargs.get('wantvar', False):
            raise NotImplementedError('wantvar is broken in the reference as well (lsqr.py:155)')
        window = kwargs.get('window', 5)
        store_iterates = kwargs.get('store_iterates', False)
        table = kwargs.get('_table')                         # `show=True`: the reference's iteration log (see _ShowTable)
        b = as_f64_vector(np.asarray(rhs).squeeze()[:m], m, 'rhs')
        At = A.T
        self.iterates = []
        # (no placement draws: they pay for CG's fused passes only)
        with DeviceRun(A, self.kind, b, transpose=At, sides=[payload for _, payload in sides], placement_draws=1,
                       itnlim=int(itnlim), damp=float(damp), atol=float(atol), btol=float(btol), conlim=float(conlim),
                       etol=float(kwargs.get('etol', 1.0e-6)), window=int(window)) as run:
            run.setup()
            res = run.finish()
            if store_iterates:
                self.iterates.append(run.x())
            if table is not None:
                table.start(res, run.x_first())
            while not res.halted:
                run.iterate(1 if (store_iterates or table is not None) else (1 << 20))
                last_itn = int(res.itn)
                res = run.finish()
                advanced = int(res.itn) > last_itn
                if store_iterates and advanced:
                    self.iterates.append(run.x())
                if table is not None:
                    table.after_pass(res, run.x_first() if advanced else None, advanced)
            x = run.x()
            hist, derr = run.history(), run.history2()
            r = run.vector(0) if self.kind == _lib.MK_CRAIG else None
        itn = int(res.itn)
        A._nMatvec += itn
        At._nMatvec += itn + (1 if res.residNorm0 > 0 else 0)
        self._hist = hist
        self.dir_errors_window = [np.float64(e) for e in derr[window:]]
        return res, x, r, itn


class _ShowTable(object):
    """The iteration log the reference prints with ``show=True`` (lsqr.py:222-234,394-411; lsmr.py:288-296,450-473), from
    the device loop stepped one pass at a time.  One quantity of a row is only settled by the NEXT pass's gate kernel
    (LSQR: cond(A), lsqr.py:338; LSMR: norm(x) for the print rule, lsmr.py:415), so row k is printed after pass k + 1 --
    or after the halting gate -- from the snapshot taken after pass k.  Same print rule, same formats; costs a device
    round trip per iteration, like every `show` mode: a debugging aid."""

    def __init__(self, kind, n, itnlim, atol, btol, ctol=0.0, pfreq=20):
        self.kind, self.n, self.itnlim, self.atol, self.btol, self.ctol = kind, n, itnlim, atol, btol, ctol
        self.pending = None
        self.pfreq, self.pcount = pfreq, 0
        self.lsqr = kind == _lib.MK_LSQR
        self.head = ('   Itn      x(1)       r1norm     r2norm ' + ' Compatible   LS      Norm A   Cond A') if self.lsqr else \
            ('   itn      x(1)       norm r    norm Ar ' + ' compatible   LS      norm A   cond A')

    @staticmethod
    def _snap(res, x0):
        return dict(itn=int(res.itn), x0=x0, r1=res.aux[0], r2=res.residNorm, normr=res.aux[1], normar=res.aux[2],
                    Anorm=res.Anorm, Acond=res.Acond, Arnorm=res.Arnorm, xnorm=res.xnorm, bnorm=res.residNorm0,
                    istop=int(res.istop))

    def start(self, res, x0):
        s = self._snap(res, x0)
        if res.halted:                                       # x = 0 is the solution: the reference prints msg[0] and returns
            return
        print(' ')
        print(self.head)
        beta = s['bnorm']
        if self.lsqr:                                        # lsqr.py:229-234 (test2 = alpha / beta; Arnorm = alpha beta)
            print('%6g %12.5e' % (0, x0) + ' %10.3e %10.3e' % (s['r1'], s['r2']) + '  %8.1e %8.1e' % (1.0, s['Arnorm'] / beta / beta))
        else:                                                # lsmr.py:291-296 (normA = alpha at this point)
            print(''.join(['%6g %12.5e' % (0, x0), ' %10.3e %10.3e' % (s['normr'], s['normar']),
                           '  %8.1e %8.1e' % (1, s['Anorm'] / beta)]))

    def _row(self, s, late):
        itn, bnorm = s['itn'], s['bnorm']
        if self.lsqr:
            Acond = late['Acond']                            # settled by the gate that followed
            test1 = s['r2'] / bnorm
            test2 = np.inf if (s['Anorm'] == 0. or s['r2'] == 0.) else s['Arnorm'] / (s['Anorm'] * s['r2'])
            test3 = np.inf if Acond == 0.0 else 1.0 / Acond
            rtol = self.btol + self.atol * s['Anorm'] * s['xnorm'] / bnorm
            prnt = (self.n <= 40 or itn <= 10 or itn >= self.itnlim - 10 or itn % 10 == 0 or test3 <= 2 * 0.0
                    or test2 <= 10 * self.atol or test1 <= 10 * rtol or late['istop'] != 0)     # (ctol stays 0: lsqr.py:161-163)
            if prnt:
                print('%6g %12.5e' % (itn, s['x0']) + ' %10.3e %10.3e' % (s['r1'], s['r2']) + '  %8.1e %8.1e' % (test1, test2)
                      + ' %8.1e %8.1e' % (s['Anorm'], Acond))
        else:
            normx = late['xnorm']
            test1 = s['normr'] / bnorm
            test2 = s['normar'] / (s['Anorm'] * s['normr'])
            test3 = 1 / s['Acond']
            rtol = self.btol + self.atol * s['Anorm'] * normx / bnorm
            prnt = (self.n <= 40 or itn <= 10 or itn >= self.itnlim - 10 or itn % 10 == 0 or test3 <= 1.1 * self.ctol
                    or test2 <= 1.1 * self.atol or test1 <= 1.1 * rtol or late['istop'] != 0)
            if prnt:
                if self.pcount >= self.pfreq:
                    self.pcount = 0
                    print(' ')
                    print(self.head)
                self.pcount += 1
                print(''.join(['%6g %12.5e' % (itn, s['x0']), ' %10.3e %10.3e' % (s['normr'], s['normar']),
                               '  %8.1e %8.1e' % (test1, test2), ' %8.1e %8.1e' % (s['Anorm'], s['Acond'])]))

    def after_pass(self, res, x0, advanced):
        now = self._snap(res, x0)
        if self.pending is not None and (advanced or res.halted):
            late = dict(now, istop=now['istop'] if res.halted and not advanced else 0)
            self._row(self.pending, late)
            self.pending = None
        if advanced:
            self.pending = now
            if res.halted:                                   # (a pass and its halting gate in one call)
                self._row(now, now)
                self.pending = None


class LSQRFramework(_LlsBase):
    """LSQR for ``A x = b`` / ``min |b - A x|`` / damped least squares (lsqr.py:26-453).

    Result attributes: `x, bestSolution, istop, itn, nMatvec (= 2 itn), r1norm, r2norm, residNorm, Anorm,
    Acond, Arnorm, xnorm, var (None), optimal, status`.
    """
    kind = _lib.MK_LSQR

    def solve(self, rhs, itnlim=0, damp=0.0, M=None, N=None, atol=1.0e-9, btol=1.0e-9, conlim=1.0e+8,
              show=False, wantvar=False, **kwargs):
        m, n = self.A.shape
        if itnlim == 0:
            itnlim = 3 * n
        kwargs['wantvar'] = wantvar
        if show:                                             # lsqr.py:168-175
            print(' ')
            print('LSQR            Least-squares solution of  Ax = b')
            print('The matrix A has %8d rows and %8d cols' % (m, n))
            print('damp = %20.14e     wantvar = %-5s' % (damp, repr(wantvar)))
            print('atol = %8.2e                 conlim = %8.2e' % (atol, conlim))
            print('btol = %8.2e                 itnlim = %8g' % (btol, itnlim))
            kwargs['_table'] = _ShowTable(self.kind, n, itnlim, atol, btol)
        res, x, _, itn = self._run(rhs, itnlim, damp, atol, btol, conlim, M, N, kwargs)
        if kwargs.get('store_resids', False):
            self.resids = [np.float64(res.residNorm0)] + [np.float64(h) for h in self._hist]
        istop = int(res.istop)
        if show and istop == 0:
            print(self.msg[0])                               # lsqr.py:215
        elif show:                                           # lsqr.py:418-434
            print(' ')
            print('LSQR finished')
            print(self.msg[istop])
            print(' ')
            print('istop =%8g   r1norm =%8.1e' % (istop, res.aux[0]) + '   ' + 'Anorm =%8.1e   Arnorm =%8.1e' % (res.Anorm, res.Arnorm))
            print('itn   =%8g   r2norm =%8.1e' % (itn, res.residNorm) + '   ' + 'Acond =%8.1e   xnorm  =%8.1e' % (res.Acond, res.xnorm))
            print('                  bnorm  =%8.1e' % res.residNorm0)
            print('xNrgNorm2 = %7.1e   trnDirErr = %7.1e' % (res.aux[3], self._trnc_dir_err(res)))
            print(' ')
        self.status = _STATUS[istop]
        self.optimal = istop in [1, 2, 4, 5, 8]
        self.x = self.bestSolution = x
        self.istop = istop
        self.itn = itn
        self.nMatvec = 2 * itn
        self.r1norm = np.float64(res.aux[0])
        self.r2norm = np.float64(res.residNorm)
        self.residNorm = self.r2norm
        self.Anorm = np.float64(res.Anorm)
        self.Acond = np.float64(res.Acond)
        self.Arnorm = np.float64(res.Arnorm)
        self.xnorm = np.float64(res.xnorm)
        self.var = None
        return


class LSMRFramework(_LlsBase):
    """LSMR (lsmr.py:28-492).  Like the reference, `solve` RETURNS
    ``(x, istop, itn, normr, normar, normA, condA, normx)`` and only sets `self.x`."""
    kind = _lib.MK_LSMR

    def solve(self, b, damp=0.0, atol=1e-9, btol=1e-9, conlim=1e8, M=None, N=None, itnlim=None, show=False,
              **kwargs):
        m, n = getattr(self.A, 'global_shape', self.A.shape)    # (row blocks on several GPUs: the same limit everywhere)
        if itnlim is None:
            itnlim = min([m, n])
        if show:                                             # lsmr.py:196-206
            print(' ')
            print('LSMR            Least-squares solution of  Ax = b')
            print('The matrix A has %8g rows  and %8g cols' % (m, n))
            print('damp = %20.14e' % (damp))
            print('atol = %8.2e                 conlim = %8.2e' % (atol, conlim))
            print('btol = %8.2e               itnlim = %8g' % (btol, itnlim))
            kwargs['_table'] = _ShowTable(self.kind, n, itnlim, atol, btol, ctol=(1.0 / conlim if conlim > 0 else 0.0))
        res, x, _, itn = self._run(b, itnlim, damp, atol, btol, conlim, M, N, kwargs)
        istop = int(res.istop)
        if kwargs.get('store_resids', False):
            self.resids = [np.float64(res.residNorm0)] + [np.float64(h) for h in self._hist]
        if show and istop == 0 and itn == 0:
            print(self.msg[0])                               # lsmr.py:286
        elif show:                                           # lsmr.py:479-489
            print(' ')
            print('LSMR finished')
            print(self.msg[istop])
            print('istop =%8g    normr =%8.1e' % (istop, res.aux[1]), '    normA =%8.1e    normAr =%8.1e' % (res.Anorm, res.aux[2]))
            print('itn   =%8g    condA =%8.1e' % (itn, res.Acond), '    normx =%8.1e' % (res.xnorm))
            print('Estimated energy norm of x: %7.1e' % np.sqrt(res.aux[3]))
        self.x = x
        return (x, istop, itn, np.float64(res.aux[1]), np.float64(res.aux[2]), np.float64(res.Anorm),
                np.float64(res.Acond), np.float64(res.xnorm))


class CRAIGFramework(_LlsBase):
    """CRAIG (craig.py:30-520).  Result attributes: `x, bestSolution, r, istop, itn, nMatvec, r1norm, r2norm,
    Arnorm, xnorm, optimal, status`."""
    kind = _lib.MK_CRAIG

    def solve(self, rhs, itnlim=0, damp=0.0, M=None, N=None, atol=1.0e-9, btol=1.0e-9, conlim=1.0e+8,
              show=False, wantvar=False, **kwargs):
        m, n = self.A.shape
        if itnlim == 0:
            itnlim = 3 * n
        kwargs['wantvar'] = wantvar
        if show:                                             # craig.py:193-200 (its iteration log is commented out there)
            print(' ')
            print('CRAIG           Least-squares solution of  Ax = b')
            print('The matrix A has %8d rows and %8d cols' % (m, n))
            print('damp = %20.14e     wantvar = %-5s' % (damp, repr(wantvar)))
            print('atol = %8.2e                 conlim = %8.2e' % (atol, conlim))
            print('btol = %8.2e                 itnlim = %8g' % (btol, itnlim))
        res, x, r, itn = self._run(rhs, itnlim, damp, atol, btol, conlim, M, N, kwargs)
        istop = int(res.istop)
        if show and istop == 0:
            print(self.msg[0])                               # craig.py:239
        elif show:                                           # craig.py:483-499
            print(' ')
            print('CRAIG finished')
            print(self.msg[istop])
            print(' ')
            print('istop =%8g   r1norm =%8.1e' % (istop, res.aux[0]))
            print('itn   =%8g   r2norm =%8.1e' % (itn, res.residNorm))
            print('                  bnorm  =%8.1e' % res.residNorm0)
            print('xNrgNorm2 = %7.1e   trnDirErr = %7.1e' % (res.aux[3], self._trnc_dir_err(res)))
            print(' ')
        self.dir_errors_d_window = self.dir_errors_window
        self.status = _STATUS[istop]
        self.optimal = istop in [1, 2, 4, 5, 8]
        self.x = self.bestSolution = x
        self.r = r
        self.istop = istop
        self.itn = itn
        self.nMatvec = 2 * itn
        self.r1norm = np.float64(res.aux[0])
        self.r2norm = np.float64(res.residNorm)
        self.Arnorm = np.float64(res.Arnorm)
        self.xnorm = np.float64(res.xnorm)
        return


class CRAIGMRFramework(_LlsBase):
    """CRAIG-MR (craigmr.py:12-241; its per-iteration debugging print at :190 is dropped).  `x` has
    ``nargout`` entries as in the reference (craigmr.py:112)."""
    kind = _lib.MK_CRAIGMR

    def solve(self, b, damp=0.0, atol=1e-9, btol=1e-9, conlim=1e8, M=None, N=None, itnlim=None, show=False,
              **kwargs):
        m, n = getattr(self.A, 'global_shape', self.A.shape)
        if itnlim is None:
            itnlim = min([m, n])
        res, x, _, itn = self._run(b, itnlim, damp, atol, btol, conlim, M, N, kwargs)
        istop = int(res.istop)
        if show:
            print(' ')
            print('CRAIG-MR finished')
            print(self.msg[istop])
        self.status = _STATUS[istop]
        self.optimal = istop in [1, 2, 4, 5, 8]
        self.x = self.bestSolution = x
        self.istop = istop
        self.itn = itn
        self.nMatvec = 2 * itn
        return
