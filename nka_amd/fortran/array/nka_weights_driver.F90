!! nka_weights_driver -- diagonal dot-product weights through the FORTRAN front end (a%set_dot_weights for a host array,
!! a%set_dot_weights_dev for device memory; module nka_type -> iso_c_binding -> libnka_hip.so).
!!
!!   nka_weights_driver [N [MVEC [CALLS [FLAVOR]]]]      defaults 100003 6 14 2
!!
!! Six accelerators, the same input stream:
!!   P   no weights, on x
!!   U1  w == 1 set from a host array,    on x        U1D  w == 1 set from device memory, on x
!!   W4  w == 4 set from a host array,    on x / 2    W4D  w == 4 set from device memory, on x / 2
!!   C   b = W4D (deep copy) after call 5, then on x / 2 like W4D
!! w == 4 on x / 2 is the plain run on x scaled by exact powers of two (include/nka_hip.h), so every state digest equals P's
!! and the returned f equals P's / 2, bit for bit.  Prints one line per call, "digests T d_P d_U1 d_U1D d_W4 d_W4D d_C" (the
!! copy's column repeats W4D's until it exists), then "OK"; stops with an error at the first difference.

program nka_weights_driver

  use, intrinsic :: iso_fortran_env, only: r8 => real64, i8 => int64
  use, intrinsic :: iso_c_binding
  use nka_hip_c
  use nka_type
  implicit none

  integer(i8) :: n = 100003_i8
  integer :: mvec = 6, calls = 14, flavor = NKA_HIP_FLAVOR_C
  character(64) :: arg
  type(nka) :: p, u1, u1d, w4, w4d, c
  type(c_ptr) :: ws, ones_dev, fours_dev
  real(r8), allocatable :: x(:), fp(:), fu1(:), fu1d(:), fw4(:), fw4d(:), fc(:), wgt(:)
  integer(c_int64_t) :: d(6)
  integer :: t

  if (command_argument_count() >= 1) then; call get_command_argument(1, arg); read(arg,*) n; end if
  if (command_argument_count() >= 2) then; call get_command_argument(2, arg); read(arg,*) mvec; end if
  if (command_argument_count() >= 3) then; call get_command_argument(3, arg); read(arg,*) calls; end if
  if (command_argument_count() >= 4) then; call get_command_argument(4, arg); read(arg,*) flavor; end if

  allocate(x(n), fp(n), fu1(n), fu1d(n), fw4(n), fw4d(n), fc(n), wgt(n))
  call nka_hip_check(nka_hip_vec_workspace_create(ws, 0_c_int32_t, c_null_ptr), 'vec_workspace_create')
  call nka_hip_check(nka_hip_vec_alloc(ws, n, ones_dev), 'vec_alloc')
  call nka_hip_check(nka_hip_vec_alloc(ws, n, fours_dev), 'vec_alloc')
  call p%init(int(n), mvec, flavor=flavor)
  call u1%init(int(n), mvec, flavor=flavor)
  call u1d%init(int(n), mvec, flavor=flavor)
  call w4%init(int(n), mvec, flavor=flavor)
  call w4d%init(int(n), mvec, flavor=flavor)
  wgt = 1.0_r8
  call u1%set_dot_weights(wgt)
  call nka_hip_check(nka_hip_vec_h2d(ws, n, ones_dev, wgt), 'vec_h2d')
  call u1d%set_dot_weights_dev(ones_dev)
  wgt = 4.0_r8
  call w4%set_dot_weights(wgt)
  call nka_hip_check(nka_hip_vec_h2d(ws, n, fours_dev, wgt), 'vec_h2d')
  call w4d%set_dot_weights_dev(fours_dev)
  wgt = -1.0_r8                  ! the library holds copies: the caller's arrays are free again
  call nka_hip_check(nka_hip_vec_h2d(ws, n, fours_dev, wgt), 'vec_h2d')
  if (p%dot_weighted() .or. .not. (u1%dot_weighted() .and. u1d%dot_weighted() .and. w4%dot_weighted() &
      .and. w4d%dot_weighted())) error stop 'dot_weighted() does not report what was set'

  do t = 1, calls
    call random_number(x)
    x = 2.0_r8*x - 1.0_r8
    fp = x; fu1 = x; fu1d = x
    fw4 = 0.5_r8*x; fw4d = 0.5_r8*x; fc = 0.5_r8*x
    call p%accel_update(fp)
    call u1%accel_update(fu1)
    call u1d%accel_update(fu1d)
    call w4%accel_update(fw4)
    call w4d%accel_update(fw4d)
    if (t > 5) call c%accel_update(fc)
    d(1) = p%state_digest()
    d(2) = u1%state_digest()
    d(3) = u1d%state_digest()
    d(4) = w4%state_digest()
    d(5) = w4d%state_digest()
    d(6) = d(5)
    if (t > 5) d(6) = c%state_digest()
    write(*, '(a, i0, 6(1x, i0))') 'digests ', t, d
    if (any(d /= d(1))) error stop 'state digests differ'
    if (any(fu1 /= fp) .or. any(fu1d /= fp)) error stop 'w == 1: f differs from the plain run'
    if (any(2.0_r8*fw4 /= fp) .or. any(2.0_r8*fw4d /= fp)) error stop 'w == 4 on x/2: f is not the plain run / 2'
    if (t > 5) then
      if (any(fc /= fw4d)) error stop 'the deep copy differs from its source'
    end if
    if (t == 5) then
      c = w4d                                  ! deep copy: the weights travel with the object
      if (.not. c%dot_weighted()) error stop 'the deep copy lost the weights'
    end if
  end do
  print '(a)', 'OK'

end program
