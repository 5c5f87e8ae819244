! `polynomial`: the public surface of src/nonlin_polynomials.f90:8-72 -- initialize, order, fit, fit_thru_zero, evaluate
! (real and complex argument), companion_mtx, roots, get, get_all, set, divide, assignment(=) (from a polynomial, a number,
! an array), operator(+), operator(-), operator(*) (polynomial x polynomial, polynomial x number, number x polynomial)
! and the polynomial(order) / polynomial(c) constructors.  The two fits marshal to nlh_poly_fit -- Vandermonde panel,
! Householder QR and back substitution on the GPU (:146-238); roots marshals to nlh_poly_roots -- balancing and
! double-shift QR on the companion matrix on the GPU (:357-381), so it is not `pure` as the reference declares it.
! The arithmetic is host code that keeps the reference's results statement by statement, including where they are odd:
! for x of higher order than y, x + y and x - y leave the leading coefficient 0 (:538, :593), and x - y with x
! uninitialised is +y (:576-580).
!
! Representation: `cf(0:deg)`, cf(k) multiplying x**k; an object that was never initialised has no `cf` and reports
! order -1 exactly as the reference does (:112-143).
module nonlin_polynomials
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin_error_handling, only : NL_INVALID_OPERATION_ERROR, NL_INDEX_OUT_OF_RANGE_ERROR, NL_DIVIDE_BY_ZERO_ERROR
    use nonlin_hip_c
    implicit none
    private
    public :: polynomial
    public :: assignment(=)
    public :: operator(+)
    public :: operator(-)
    public :: operator(*)

    interface assignment(=)
        module procedure :: pl_copy
        module procedure :: pl_fill
        module procedure :: pl_take_array
    end interface

    interface operator(+)
        module procedure :: pl_sum
    end interface

    interface operator(-)
        module procedure :: pl_difference
    end interface

    interface operator(*)
        module procedure :: pl_product
        module procedure :: pl_times_number
        module procedure :: pl_number_times
    end interface

    type polynomial
        real(real64), private, allocatable :: cf(:)          ! cf(0:deg)
    contains
        generic, public :: initialize => pl_alloc, pl_from_coefs
        procedure, public :: order => pl_degree
        procedure, public :: fit => pl_fit_free
        procedure, public :: fit_thru_zero => pl_fit_origin
        generic, public :: evaluate => pl_horner, pl_horner_cx
        procedure, public :: companion_mtx => pl_companion
        procedure, public :: roots => pl_roots
        procedure, public :: get => pl_coef
        procedure, public :: get_all => pl_coefs
        procedure, public :: set => pl_put
        procedure, public :: divide => pl_long_division
        procedure, private :: pl_horner
        procedure, private :: pl_horner_cx
        procedure, private :: pl_alloc
        procedure, private :: pl_from_coefs
    end type

    interface polynomial
        module procedure :: pl_new_zero
        module procedure :: pl_new_from
    end interface

contains
    ! zero polynomial of the given order (:69-90; a negative order is the reference's NL_INVALID_INPUT_ERROR there,
    ! reported here by the same small integer the shim uses for size errors)
    pure subroutine pl_alloc(this, order)
        class(polynomial), intent(inout) :: this
        integer(int32), intent(in) :: order
        if (order < 0) error stop 2
        if (allocated(this%cf)) deallocate(this%cf)
        allocate(this%cf(0:order), source = 0.0d0)
    end subroutine

    ! from a coefficient array, lowest power first (:93-109)
    pure subroutine pl_from_coefs(this, c)
        class(polynomial), intent(inout) :: this
        real(real64), intent(in), dimension(:) :: c
        if (size(c) < 1) error stop 2
        if (allocated(this%cf)) deallocate(this%cf)
        allocate(this%cf(0:size(c) - 1))
        this%cf(0:) = c
    end subroutine

    pure integer(int32) function pl_degree(this) result(deg)
        class(polynomial), intent(in) :: this
        deg = -1
        if (allocated(this%cf)) deg = ubound(this%cf, 1)
    end function

    ! both fits: size checks of :159-166 / :206-213, then the device
    subroutine pl_fit_front(this, x, y, order, origin)
        class(polynomial), intent(inout) :: this
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(inout), dimension(:) :: y
        integer(int32), intent(in) :: order
        logical, intent(in) :: origin
        integer(c_int) :: rc
        integer(c_int32_t) :: npts
        real(c_double), allocatable :: xs(:), ys(:), sol(:)
        npts = int(size(x), c_int32_t)
        if (size(y) /= npts) error stop 3
        if (order < 1 .or. order >= npts) error stop 4
        allocate(xs(npts), source = x)
        allocate(ys(npts), source = y)
        allocate(sol(0:order))
        rc = nlh_poly_fit(nlh_default_handle(), npts, order, merge(1, 0, origin), xs, ys, sol)
        if (rc /= 0) error stop rc
        if (pl_degree(this) /= order) call pl_alloc(this, order)
        this%cf = sol
    end subroutine

    subroutine pl_fit_free(this, x, y, order)               ! :146-190
        class(polynomial), intent(inout) :: this
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(inout), dimension(:) :: y
        integer(int32), intent(in) :: order
        call pl_fit_front(this, x, y, order, .false.)
    end subroutine

    subroutine pl_fit_origin(this, x, y, order)             ! :193-238
        class(polynomial), intent(inout) :: this
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(inout), dimension(:) :: y
        integer(int32), intent(in) :: order
        call pl_fit_front(this, x, y, order, .true.)
    end subroutine

    ! Horner from the leading coefficient down: the operations of :241-268 in the same order (its first line is this
    ! loop's first trip), 0 for an uninitialised object
    pure elemental function pl_horner(this, x) result(y)
        class(polynomial), intent(in) :: this
        real(real64), intent(in) :: x
        real(real64) :: y
        integer(int32) :: k
        y = 0.0d0
        if (.not. allocated(this%cf)) return
        y = this%cf(ubound(this%cf, 1))
        do k = ubound(this%cf, 1) - 1, 0, -1
            y = y * x + this%cf(k)
        end do
    end function

    ! coefficient `ind` (1-based: c(1) + c(2) x + ...).  Asking an uninitialised polynomial for a coefficient is an
    ! invalid operation in the reference (:399) -- it stops; so does this.
    pure function pl_coef(this, ind) result(c)
        class(polynomial), intent(in) :: this
        integer(int32), intent(in) :: ind
        real(real64) :: c
        if (.not. allocated(this%cf)) error stop NL_INVALID_OPERATION_ERROR
        if (ind < 1 .or. ind > size(this%cf)) error stop NL_INDEX_OUT_OF_RANGE_ERROR
        c = this%cf(ind - 1)
    end function

    pure function pl_coefs(this) result(c)
        class(polynomial), intent(in) :: this
        real(real64), allocatable, dimension(:) :: c
        if (allocated(this%cf)) then
            allocate(c(size(this%cf)))
            c = this%cf
        else
            allocate(c(0))
        end if
    end function

    ! (:426-447: silently ignored on an uninitialised object, index checked otherwise)
    pure subroutine pl_put(this, ind, c)
        class(polynomial), intent(inout) :: this
        integer(int32), intent(in) :: ind
        real(real64), intent(in) :: c
        if (.not. allocated(this%cf)) return
        if (ind < 1 .or. ind > size(this%cf)) error stop NL_INDEX_OUT_OF_RANGE_ERROR
        this%cf(ind - 1) = c
    end subroutine

    ! Horner for a complex argument (:290-321).  The product y x is written out as (yr xr - yi xi, yr xi + yi xr) and the
    ! real coefficient joins the real part only, so the bits do not depend on how a compiler guards complex products.
    pure elemental function pl_horner_cx(this, x) result(y)
        class(polynomial), intent(in) :: this
        complex(real64), intent(in) :: x
        complex(real64) :: y
        integer(int32) :: k, deg
        real(real64) :: xr, xi, yr, yi, tr, ti
        y = (0.0d0, 0.0d0)
        if (.not. allocated(this%cf)) return
        deg = ubound(this%cf, 1)
        if (deg == 0) then
            y = cmplx(this%cf(0), 0.0d0, real64)
            return
        end if
        xr = real(x, real64)
        xi = aimag(x)
        yr = this%cf(deg) * xr + this%cf(deg - 1)
        yi = this%cf(deg) * xi
        do k = deg - 2, 0, -1
            tr = yr * xr - yi * xi
            ti = yr * xi + yi * xr
            yr = tr + this%cf(k)
            yi = ti
        end do
        y = cmplx(yr, yi, real64)
    end function

    ! the companion matrix (:324-354): -c(i) / c(n + 1) down the last column, ones below the diagonal
    pure function pl_companion(this) result(c)
        class(polynomial), intent(in) :: this
        real(real64), allocatable, dimension(:,:) :: c
        integer(int32) :: k, deg
        deg = pl_degree(this)
        if (deg < 1) then
            allocate(c(0, 0))
            return
        end if
        allocate(c(deg, deg), source = 0.0d0)
        do k = 1, deg
            c(k, deg) = -this%cf(k - 1) / this%cf(deg)
            if (k < deg) c(k + 1, k) = 1.0d0
        end do
    end function

    ! all roots (:357-381): on the device.  Order as LAPACK's DGEEV reports the eigenvalues of the companion matrix (a
    ! complex pair as (re, +im), (re, -im); exact zero roots of zero low coefficients last).  A per-polynomial failure
    ! (NL_CONVERGENCE_ERROR, NL_DIVIDE_BY_ZERO_ERROR for a zero leading coefficient, NL_INVALID_INPUT_ERROR) stops.
    function pl_roots(this) result(z)
        class(polynomial), intent(in) :: this
        complex(real64), allocatable, dimension(:) :: z
        integer(c_int) :: rc
        integer(c_int32_t) :: deg, info
        real(c_double), allocatable :: c(:), zz(:,:)
        integer(int32) :: k
        deg = pl_degree(this)
        if (deg < 1) then                                   ! :373 (and an uninitialised object: nothing to solve)
            allocate(z(0))
            return
        end if
        allocate(c(0:deg), source = this%cf)
        allocate(zz(2, deg))
        info = 0
        rc = nlh_poly_roots(nlh_default_handle(), deg, c, zz, info)
        if (rc /= 0) error stop rc
        if (info /= 0) error stop info
        allocate(z(deg))
        do k = 1, deg
            z(k) = cmplx(zz(1, k), zz(2, k), real64)
        end do
    end function

    ! ---- assignment(=), :454-498 ----
    pure subroutine pl_copy(x, y)
        class(polynomial), intent(inout) :: x
        class(polynomial), intent(in) :: y
        if (allocated(x%cf)) deallocate(x%cf)
        if (allocated(y%cf)) allocate(x%cf(0:ubound(y%cf, 1)), source = y%cf)
    end subroutine

    pure subroutine pl_fill(x, y)                            ! every coefficient; nothing on an uninitialised object
        class(polynomial), intent(inout) :: x
        real(real64), intent(in) :: y
        if (allocated(x%cf)) x%cf = y
    end subroutine

    pure subroutine pl_take_array(x, y)
        class(polynomial), intent(inout) :: x
        real(real64), intent(in), dimension(:) :: y
        call pl_from_coefs(x, y)
    end subroutine

    ! ---- operator(+) / operator(-), :501-608 ----
    pure function pl_combine(x, y, sgn) result(z)
        class(polynomial), intent(in) :: x, y
        real(real64), intent(in) :: sgn                      ! +1: x + y, -1: x - y
        type(polynomial) :: z
        integer(int32) :: dx, dy, k
        dx = pl_degree(x)
        dy = pl_degree(y)
        if (dx == -1 .and. dy == -1) return
        allocate(z%cf(0:max(dx, dy)), source = 0.0d0)
        if (dx == -1) then
            z%cf = y%cf                                      ! :523, and :578 for the difference: +y
        else if (dy == -1) then
            z%cf = x%cf
        else if (dx > dy) then
            do k = 0, dy
                z%cf(k) = pl_pair(x%cf(k), y%cf(k), sgn)
            end do
            do k = dy + 1, dx - 1                            ! :538 / :593: the copy stops one short, cf(dx) stays 0
                z%cf(k) = x%cf(k)
            end do
        else if (dx < dy) then
            do k = 0, dx
                z%cf(k) = pl_pair(x%cf(k), y%cf(k), sgn)
            end do
            do k = dx + 1, dy
                if (sgn < 0.0d0) then
                    z%cf(k) = -y%cf(k)
                else
                    z%cf(k) = y%cf(k)
                end if
            end do
        else
            do k = 0, dx
                z%cf(k) = pl_pair(x%cf(k), y%cf(k), sgn)
            end do
        end if
    end function

    pure elemental function pl_pair(a, b, sgn) result(c)
        real(real64), intent(in) :: a, b, sgn
        real(real64) :: c
        if (sgn < 0.0d0) then
            c = a - b
        else
            c = a + b
        end if
    end function

    pure function pl_sum(x, y) result(z)
        class(polynomial), intent(in) :: x, y
        type(polynomial) :: z
        z = pl_combine(x, y, 1.0d0)
    end function

    pure function pl_difference(x, y) result(z)
        class(polynomial), intent(in) :: x, y
        type(polynomial) :: z
        z = pl_combine(x, y, -1.0d0)
    end function

    ! ---- operator(*), :611-678 ----
    pure function pl_product(x, y) result(z)
        class(polynomial), intent(in) :: x, y
        type(polynomial) :: z
        integer(int32) :: i, j, dx, dy
        dx = pl_degree(x)
        dy = pl_degree(y)
        call pl_alloc(z, dx + dy)
        do i = 0, dx
            do j = 0, dy
                z%cf(i + j) = z%cf(i + j) + x%cf(i) * y%cf(j)
            end do
        end do
    end function

    pure function pl_times_number(x, y) result(z)
        class(polynomial), intent(in) :: x
        real(real64), intent(in) :: y
        type(polynomial) :: z
        call pl_alloc(z, pl_degree(x))
        z%cf = x%cf * y
    end function

    pure function pl_number_times(x, y) result(z)
        real(real64), intent(in) :: x
        class(polynomial), intent(in) :: y
        type(polynomial) :: z
        call pl_alloc(z, pl_degree(y))
        z%cf = y%cf * x
    end function

    ! ---- divide, :681-779: long division; quotient and remainder trimmed of leading coefficients <= epsilon ----
    pure subroutine pl_long_division(numerator, divisor, quotient, remainder)
        class(polynomial), intent(in) :: numerator, divisor
        type(polynomial), intent(out) :: quotient, remainder
        integer(int32) :: i, j, n, m
        real(real64) :: coeff, lead
        real(real64), allocatable :: q(:), r(:)
        call pl_alloc(quotient, 0)
        call pl_alloc(remainder, 0)
        if (.not. allocated(numerator%cf)) error stop 1
        if (.not. allocated(divisor%cf)) error stop 2
        n = ubound(numerator%cf, 1)
        m = ubound(divisor%cf, 1)
        lead = divisor%cf(m)
        if (abs(lead) <= epsilon(lead)) error stop NL_DIVIDE_BY_ZERO_ERROR
        if (n < m) then
            call pl_from_coefs(remainder, numerator%cf)
            return
        end if
        allocate(q(0:n - m), source = 0.0d0)
        allocate(r(0:n), source = numerator%cf)
        do i = n - m, 0, -1
            coeff = r(i + m) / lead
            q(i) = coeff
            do j = 0, m
                r(i + j) = r(i + j) - coeff * divisor%cf(j)
            end do
        end do
        call pl_trimmed(quotient, q)
        call pl_trimmed(remainder, r)
    end subroutine

    ! v(0:) without its leading coefficients of magnitude <= epsilon; the zero polynomial of order 0 if none is left
    pure subroutine pl_trimmed(p, v)
        type(polynomial), intent(inout) :: p
        real(real64), intent(in) :: v(0:)
        integer(int32) :: k, top
        top = -1
        do k = ubound(v, 1), 0, -1
            if (abs(v(k)) > epsilon(v(k))) then
                top = k
                exit
            end if
        end do
        if (top == -1) then
            call pl_alloc(p, 0)
        else
            call pl_from_coefs(p, v(0:top))
        end if
    end subroutine

    ! ---- constructors, :782-804 ----
    function pl_new_zero(order) result(p)
        integer(int32), intent(in) :: order
        type(polynomial) :: p
        call pl_alloc(p, order)
    end function

    function pl_new_from(c) result(p)
        real(real64), intent(in), dimension(:) :: c
        type(polynomial) :: p
        call pl_from_coefs(p, c)
    end function
end module
