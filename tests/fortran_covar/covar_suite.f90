! least_squares_solver%covariance / covariance_batch through the Fortran shim (nonlin_amd/fortran): the parameter covariance
! of a fit, on the three residual forms `solve` accepts -- a host callback (README Example 2, the 21 x 4 cubic fit), a
! user's device function registered with set_device_fcn, and a batch of them (device_model_batch).
! Reads the spectra written by tests/test_gpu_covar.py (stream binary: nprob, m, n (int32), t(m,nprob), y(m,nprob),
! x(n,nprob)); prints, per case, a label and the bit patterns of its numbers (the rank as a real):
!   <label> <hex> ...
! which the test compares with tests/covar_restatement.py on the CPU oracle's factorisation.
module covar_problems
    use iso_fortran_env
    implicit none
contains
    subroutine cubicfit(x, f, args)
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(out), dimension(:) :: f
        class(*), intent(inout), optional :: args
        real(real64), dimension(21) :: xp, yp
        xp = [0.0d0, 0.1d0, 0.2d0, 0.3d0, 0.4d0, 0.5d0, 0.6d0, 0.7d0, 0.8d0, &
            0.9d0, 1.0d0, 1.1d0, 1.2d0, 1.3d0, 1.4d0, 1.5d0, 1.6d0, 1.7d0, &
            1.8d0, 1.9d0, 2.0d0]
        yp = [1.216737514d0, 1.250032542d0, 1.305579195d0, 1.040182335d0, &
            1.751867738d0, 1.109716707d0, 2.018141531d0, 1.992418729d0, &
            1.807916923d0, 2.078806005d0, 2.698801324d0, 2.644662712d0, &
            3.412756702d0, 4.406137221d0, 4.567156645d0, 4.999550779d0, &
            5.652854194d0, 6.784320119d0, 8.307936836d0, 8.395126494d0, &
            10.30252404d0]
        f = x(1) * xp**3 + x(2) * xp**2 + x(3) * xp + x(4) - yp
    end subroutine
end module

program covar_suite
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin
    use covar_problems
    implicit none

    interface   ! the user's library (tests/device_model/user_models.hip)
        function lorentz_create(nprob, m, t, y) bind(C, name="lorentz_create") result(ctx)
            import :: c_ptr, c_int32_t, c_double
            integer(c_int32_t), value :: nprob, m
            real(c_double), intent(in) :: t(*), y(*)
            type(c_ptr) :: ctx
        end function
        subroutine lorentz_destroy(ctx) bind(C, name="lorentz_destroy")
            import :: c_ptr
            type(c_ptr), value :: ctx
        end subroutine
        function lorentz_launch(ctx, stream, npoints, dprob, n, dx, m, df) bind(C, name="lorentz_launch") result(rc)
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: ctx, stream, dprob, dx, df
            integer(c_int32_t), value :: npoints, n, m
            integer(c_int) :: rc
        end function
    end interface

    character(len=512) :: path
    integer(int32) :: nprob, m, n, k, u, rank4
    real(real64), allocatable :: t(:,:), y(:,:), x(:,:), cov(:,:,:), sigma(:,:), chi2(:), c1(:,:), s1(:)
    integer(int32), allocatable :: rank(:)
    real(real64) :: x4(4), f21(21), cov4(4,4), sig4(4), q4, xkeep(4)
    type(c_ptr) :: ctx, ctx1
    type(vecfcn_helper) :: obj, dobj          ! a host callback; a device function (a helper holds one or the other)
    type(device_model_batch) :: batch
    type(least_squares_solver) :: lm
    type(iteration_behavior) :: ib
    procedure(vecfcn), pointer :: fcn

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m, n
    allocate(t(m, nprob), y(m, nprob), x(n, nprob))
    read(u) t
    read(u) y
    read(u) x
    close(u)

    ! ---- README Example 2: solve, then ask how well each coefficient is determined
    fcn => cubicfit
    call obj%set_fcn(fcn, 21, 4)
    x4 = 1.0d0
    call lm%solve(obj, x4, f21, ib)
    xkeep = x4
    call lm%covariance(obj, x4, cov4, sig4, rank4, q4)
    if (any(x4 /= xkeep)) error stop 10                        ! x is not changed
    print '(A,*(1X,Z16.16))', "readme_x", x4
    print '(A,*(1X,Z16.16))', "readme_cov", cov4
    print '(A,*(1X,Z16.16))', "readme_sigma", sig4
    print '(A,*(1X,Z16.16))', "readme_rank_chi2", real(rank4, real64), q4
    call lm%covariance(obj, x4, cov4, scaled = .false., tol = 1.0d-10)     ! the optional arguments left out
    print '(A,*(1X,Z16.16))', "readme_cov_unscaled", cov4

    ! ---- a user's device function, one problem through the same call
    ctx1 = lorentz_create(1, m, t(:,1), y(:,1))
    if (.not.c_associated(ctx1)) error stop 3
    call dobj%set_device_fcn(c_funloc(lorentz_launch), ctx1, m, n)
    if (.not.dobj%is_device_model_defined()) error stop 5
    allocate(c1(n, n), s1(n))
    call lm%covariance(dobj, x(:,1), c1, s1, rank4, q4)
    print '(A,*(1X,Z16.16))', "dev_one_cov", c1
    print '(A,*(1X,Z16.16))', "dev_one_sigma", s1
    print '(A,*(1X,Z16.16))', "dev_one_rank_chi2", real(rank4, real64), q4
    call dobj%clear_device_model()
    call lorentz_destroy(ctx1)

    ! ---- every problem in one call
    ctx = lorentz_create(nprob, m, t, y)
    if (.not.c_associated(ctx)) error stop 4
    call batch%create_from_device_fcn(c_funloc(lorentz_launch), ctx, nprob, m, n)
    allocate(cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    call lm%covariance_batch(batch, x, cov, sigma, rank, chi2)
    do k = 1, nprob
        print '(A,I0,*(1X,Z16.16))', "dev_batch_cov_", k, cov(:,:,k)
        print '(A,I0,*(1X,Z16.16))', "dev_batch_sigma_", k, sigma(:,k)
        print '(A,I0,*(1X,Z16.16))', "dev_batch_rank_chi2_", k, real(rank(k), real64), chi2(k)
    end do
    call lm%covariance_batch(batch, x, cov, scaled = .false.)
    print '(A,*(1X,Z16.16))', "dev_batch_unscaled_1", cov(:,:,1)
    call batch%destroy()
    call lorentz_destroy(ctx)
    print '(A)', "done"
end program
