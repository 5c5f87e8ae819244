! Exercises the shim's `polynomial` the way the reference's tests/nonlin_test_poly.f90 (roots, +, -, *, divide) and
! examples/nonlin_poly_roots_example.f90 use the type, through `use nonlin` only.  Each output line is a name followed by
! numbers as hexadecimal bit patterns (Z16.16); tests/test_gpu_polyroots.py compares them with the plain-Python
! restatement bit for bit and applies the reference tests' own tolerances.  A line "FAIL <what>" is a check that failed
! here; the program stops with a non-zero code on the first one.
program poly_suite
    use iso_fortran_env
    use nonlin
    implicit none
    real(real64), parameter :: tol_roots = 1.0d-6, tol = 1.0d-8
    type(polynomial) :: p, p1, p2, p3, q, r, f, blank
    complex(real64), allocatable :: rts(:), sol(:)
    real(real64), allocatable :: a(:), c1(:), c2(:), cm(:,:)
    integer(int32) :: i

    ! roots of x**3 - 4 x**2 + x + 6 (2, 3, -1): the polynomial must vanish at each to 1e-6
    p = polynomial([6.0d0, 1.0d0, -4.0d0, 1.0d0])
    rts = p%roots()
    sol = p%evaluate(rts)
    if (size(rts) /= 3) call fail("roots: count")
    do i = 1, size(sol)
        if (abs(sol(i)) > tol_roots) call fail("roots: residual")
    end do
    call put_cx("roots_test", rts)
    call put_cx("roots_test_values", sol)

    ! the roots example: assignment from an array, then roots
    f = [-1.0d0, -2.0d0, 0.0d0, 1.0d0]
    rts = f%roots()
    call put_cx("roots_example", rts)
    do i = 1, size(rts)
        print '(A,1X,F9.6,1X,F9.6)', "# example", real(rts(i)), aimag(rts(i))
    end do

    ! a zero constant coefficient: the exact root 0 comes last
    p = polynomial([0.0d0, -6.0d0, 1.0d0, 4.0d0, 1.0d0])
    rts = p%roots()
    call put_cx("roots_zero", rts)
    ! a complex pair
    p = polynomial([5.0d0, 2.0d0, 1.0d0])
    rts = p%roots()
    call put_cx("roots_pair", rts)
    ! order 0: no roots
    p = polynomial([3.0d0])
    rts = p%roots()
    if (size(rts) /= 0) call fail("roots: order 0")

    ! companion matrix
    p = polynomial([6.0d0, 1.0d0, -4.0d0, 1.0d0])
    cm = p%companion_mtx()
    if (any(shape(cm) /= [3, 3])) call fail("companion: shape")
    call put("companion", reshape(cm, [9]))

    ! addition and subtraction, orders 10 and 20 (fixed coefficients in place of random_number)
    allocate(c1(11), c2(21))
    do i = 1, 11
        c1(i) = 1.0d0 / real(i, real64) + 0.125d0 * real(mod(i * 7, 5), real64)
    end do
    do i = 1, 21
        c2(i) = 0.3d0 * real(i, real64) - 1.0d0 / real(i + 2, real64)
    end do
    p1 = polynomial(10)
    p2 = polynomial(20)
    do i = 1, 11
        call p1%set(i, c1(i))
    end do
    do i = 1, 21
        call p2%set(i, c2(i))
    end do
    p3 = p1 + p2
    a = p3%get_all()
    if (size(a) /= 21) call fail("add: order")
    do i = 1, 21
        if (i <= 11) then
            if (abs(a(i) - (c1(i) + c2(i))) > tol) call fail("add: low")
        else
            if (abs(a(i) - c2(i)) > tol) call fail("add: high")
        end if
    end do
    call put("add_10_20", a)
    p3 = p1 - p2
    a = p3%get_all()
    do i = 1, 21
        if (i <= 11) then
            if (abs(a(i) - (c1(i) - c2(i))) > tol) call fail("subtract: low")
        else
            if (abs(a(i) + c2(i)) > tol) call fail("subtract: high")
        end if
    end do
    call put("sub_10_20", a)
    ! the higher order on the left: the reference's loop leaves the leading coefficient 0
    p3 = p2 + p1
    call put("add_20_10", p3%get_all())
    p3 = p2 - p1
    call put("sub_20_10", p3%get_all())
    ! an uninitialised left side: the difference is +y
    p3 = blank - p1
    call put("sub_blank_10", p3%get_all())

    ! multiplication: (5 + 10 x**2 + 6 x**3) (1 + 2 x + 4 x**2) = 5 + 10 x + 30 x**2 + 26 x**3 + 52 x**4 + 24 x**5
    p1 = polynomial(3)
    p2 = polynomial(2)
    call p1%set(1, 5.0d0)
    call p1%set(2, 0.0d0)
    call p1%set(3, 10.0d0)
    call p1%set(4, 6.0d0)
    call p2%set(1, 1.0d0)
    call p2%set(2, 2.0d0)
    call p2%set(3, 4.0d0)
    p3 = p1 * p2
    a = p3%get_all()
    if (size(a) /= 6) call fail("multiply: order")
    if (any(abs(a - [5.0d0, 10.0d0, 30.0d0, 26.0d0, 52.0d0, 24.0d0]) > tol)) call fail("multiply")
    call put("mult", a)
    p3 = p1 * 2.5d0
    call put("mult_right", p3%get_all())
    p3 = 2.5d0 * p1
    call put("mult_left", p3%get_all())

    ! division: (x**3 + x) / (x + 1) = x**2 - x + 2, remainder -2
    p1 = polynomial([0.0d0, 1.0d0, 0.0d0, 1.0d0])
    p2 = polynomial([1.0d0, 1.0d0])
    call p1%divide(p2, q, r)
    a = q%get_all()
    if (size(a) /= 3) call fail("divide: quotient order")
    if (any(abs(a - [2.0d0, -1.0d0, 1.0d0]) > tol)) call fail("divide: quotient")
    call put("div_q", a)
    a = r%get_all()
    if (size(a) /= 1) call fail("divide: remainder order")
    if (abs(a(1) + 2.0d0) > tol) call fail("divide: remainder")
    call put("div_r", a)

    ! assignment: copy, scalar fill
    p3 = p1
    call p3%set(1, 9.0d0)
    if (p1%get(1) /= 0.0d0 .or. p3%get(1) /= 9.0d0) call fail("assignment: copy")
    p3 = 4.0d0
    if (p3%order() /= 3 .or. any(p3%get_all() /= 4.0d0)) call fail("assignment: scalar")
    print '(A)', "done"
contains
    subroutine fail(what)
        character(len=*), intent(in) :: what
        print '(A,1X,A)', "FAIL", what
        error stop 1
    end subroutine

    subroutine put(name, v)
        character(len=*), intent(in) :: name
        real(real64), intent(in) :: v(:)
        print '(A,*(1X,Z16.16))', name, v
    end subroutine

    subroutine put_cx(name, z)
        character(len=*), intent(in) :: name
        complex(real64), intent(in) :: z(:)
        integer(int32) :: k
        real(real64) :: flat(2 * size(z))
        do k = 1, size(z)
            flat(2 * k - 1) = real(z(k), real64)
            flat(2 * k) = aimag(z(k))
        end do
        call put(name, flat)
    end subroutine
end program
