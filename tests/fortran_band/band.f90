! A user program of the bands through the Fortran shim (nonlin_amd/fortran): Lorentzian curves on a plotting grid as a
! device model batch (create_curve with y = 0, so that the model's F(x) is the curve itself), then
! least_squares_solver%propagate_batch with given parameters and covariances -- the confidence band, and with a noise
! variance per problem the prediction band.
! Reads what tests/test_gpu_band_fortran.py writes (stream binary: nprob, npts, ncomp, baseline (int32), t(npts,nprob),
! x(n,nprob), cov(n,n,nprob), noise(nprob)) and prints, per problem,
!   val <k> <npts values, ES24.16>      sd <k> <npts values>      pred <k> <npts values>
! which the test compares digit for digit with DeviceSolver.curve_band for the same inputs.
program band
    use iso_fortran_env
    use nonlin
    implicit none

    character(len=512) :: path
    integer(int32) :: nprob, npts, ncomp, baseline, n, k, u
    real(real64), allocatable :: t(:,:), y(:,:), x(:,:), cov(:,:,:), noise(:), val(:,:), sd(:,:), val2(:,:), pred(:,:)
    type(device_model_batch) :: batch
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, npts, ncomp, baseline
    n = 3 * ncomp + baseline + 1
    allocate(t(npts, nprob), y(npts, nprob), x(n, nprob), cov(n, n, nprob), noise(nprob))
    read(u) t
    read(u) x
    read(u) cov
    read(u) noise
    close(u)

    y = 0.0d0
    call batch%create_curve(NLH_CURVE_LORENTZ, ncomp, baseline, t, y)
    if (batch%get_variable_count() /= n .or. batch%get_equation_count() /= npts) error stop 3

    allocate(val(npts, nprob), sd(npts, nprob), val2(npts, nprob), pred(npts, nprob))
    call lm%propagate_batch(batch, x, cov, val, sd)
    call lm%propagate_batch(batch, x, cov, val2, pred, noise)
    if (any(val2 /= val)) error stop 4
    do k = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "val", k, val(:,k)
        print '(A,1X,I0,*(ES24.16))', "sd", k, sd(:,k)
        print '(A,1X,I0,*(ES24.16))', "pred", k, pred(:,k)
    end do
    call batch%destroy()
    print '(A)', "done"
end program
